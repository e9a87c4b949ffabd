// vr_tf2d.hip — 2D transfer-function frames (vr_hip_render_tf2d): the composite frame of a TRILINEAR view whose
// classification is a table over (value, gradient magnitude), lit from the same gradient; and the feeder that places the table's rows, the
// histogram over (value bin, gradient-magnitude row) of the resident volume.  One ray-kernel family, tf2d_kernel, over the 24 rows of the
// isosurface, gradient_histogram_kernel per voxel size, and their launchers.
#include "vr_march.h"

namespace vr {

// LDS beside the brick tables: the table as given (no stored deltas: the differences are formed at use, each rounded on its own, as the
// contract's step 4 states them), the ESL words of the table, and the 128 g-dependence flags.  20 KiB; with the 50 KiB of the 64-bit address
// tables a CU still holds two workgroups of 1024 threads, with the 17 KiB of the 32-bit ones four of 512: LDS never lowers the wave count.
struct __attribute__((aligned(16))) Tf2dTables {
	f4 tf[VR_TF2D_ROWS_MAX * VR_TF_SIZE];
	uint32_t esl[VR_ESL_VOLUME_SIZE];
	uint32_t g_dependent[4];
};

// the kernel-argument segment of tf2d_kernel as a struct: its arguments in order
struct Tf2dKernelSegment { RayKernelArgs a; const void *vol; const float *table; const uint32_t *esl; Tf2dArgs d; uint32_t *out; };
typedef const Tf2dKernelSegment __attribute__((address_space(4))) *Tf2dSegment;

// the segment through the laundered kernel-argument pointer (vr_march.h clip_segment): what is read through it occupies no scalar register
// across the march
__device__ __forceinline__ Tf2dSegment tf2d_segment() {
	Tf2dSegment s = (Tf2dSegment) __builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(s));
	return s;
}

// Step 2 of the contract, which is step 1 of the lighting contract: the central differences one texel apart of the interpolated raw value
// at sample k of the ray, clamp addressing (all six fetches in bounds for every lane, live or not), each times its half extent.  The text of
// light_sample's gradient (vr_march.h), restated here so that the one gradient serves the classification and the lighting; its register
// diet is kept: one axis at a time, both fetches of an axis in flight only where the registers allow it.
template <int BPV, int ADDR, int LAYOUT, bool Q8>
__device__ __forceinline__ void tf2d_gradient(const void *vol, const RayKernelArgs &ka, const uint32_t *lut, f3 A, f3 B, float kx, float &gx, float &gy, float &gz) {
	const Tf2dSegment s = tf2d_segment();
	constexpr bool kPair = BPV == 1 && LAYOUT == kLayoutBricked && ADDR != kAddrWide;
	auto central = [&](auto axis) -> float {
		constexpr int X = decltype(axis)::value;
		float k = kx;
		asm volatile("" : "+v"(k));
		float xb = VR_FMA(k, A.x, B.x), yb = VR_FMA(k, A.y, B.y), zb = VR_FMA(k, A.z, B.z);
		const TriFetch<BPV, LAYOUT> fp = tri_issue<BPV, ADDR, LAYOUT>(vol, ka, lut, X == 0 ? xb + 1.0f : xb, X == 1 ? yb + 1.0f : yb, X == 2 ? zb + 1.0f : zb, true);
		TriFetch<BPV, LAYOUT> fm;
		if constexpr (kPair) fm = tri_issue<BPV, ADDR, LAYOUT>(vol, ka, lut, X == 0 ? xb - 1.0f : xb, X == 1 ? yb - 1.0f : yb, X == 2 ? zb - 1.0f : zb, true);
		__builtin_amdgcn_sched_barrier(0);
		asm volatile("" : "+v"(k));
		xb = VR_FMA(k, A.x, B.x); yb = VR_FMA(k, A.y, B.y); zb = VR_FMA(k, A.z, B.z);
		float vp = tri_resolve<BPV, LAYOUT, Q8>(fp, ka, X == 0 ? xb + 1.0f : xb, X == 1 ? yb + 1.0f : yb, X == 2 ? zb + 1.0f : zb);
		if constexpr (!kPair) {
			asm volatile("" : "+v"(vp), "+v"(k));
			__builtin_amdgcn_sched_barrier(0);
			xb = VR_FMA(k, A.x, B.x); yb = VR_FMA(k, A.y, B.y); zb = VR_FMA(k, A.z, B.z);
			fm = tri_issue<BPV, ADDR, LAYOUT>(vol, ka, lut, X == 0 ? xb - 1.0f : xb, X == 1 ? yb - 1.0f : yb, X == 2 ? zb - 1.0f : zb, true);
			__builtin_amdgcn_sched_barrier(0);
			asm volatile("" : "+v"(k));
			xb = VR_FMA(k, A.x, B.x); yb = VR_FMA(k, A.y, B.y); zb = VR_FMA(k, A.z, B.z);
		}
		const float vm = tri_resolve<BPV, LAYOUT, Q8>(fm, ka, X == 0 ? xb - 1.0f : xb, X == 1 ? yb - 1.0f : yb, X == 2 ? zb - 1.0f : zb);
		float g = (vp - vm) * (X == 0 ? s->a.half_x : (X == 1 ? s->a.half_y : s->a.half_z));
		asm volatile("" : "+v"(g));
		__builtin_amdgcn_sched_barrier(0);
		return g;
	};
	gx = central(std::integral_constant<int, 0>()); gy = central(std::integral_constant<int, 1>()); gz = central(std::integral_constant<int, 2>());
}

// Steps 2-4 of the lighting contract (include/vr_hip.h vr_hip_set_lighting) on the gradient the classification has used: the Blinn-Phong
// part of light_sample (vr_march.h), the same operations in the same order.  `lit` = the wave mask of the dense lanes; returns m and spec
// (1 and 0 for the lanes that are not lit): the caller forms c.xyz = fma(c.xyz, m, spec).
__device__ __forceinline__ void tf2d_blinn_phong(float gx, float gy, float gz, f3 origin, f3 dir, float kx, uint64_t lit, float cw, float &m_out, float &spec_out) {
	const Tf2dSegment s = tf2d_segment();
	const f3 pt = march_point<VR_SAMPLE_TRILINEAR>(origin, dir, kx);
	const float gg = VR_FMA(gz, gz, VR_FMA(gy, gy, gx * gx));
	lit &= __builtin_amdgcn_fcmpf(gg, 0.0f, kFcmpOGT);                          // a plateau has no surface to light
	m_out = 1.0f; spec_out = 0.0f;
	if (lit == 0ull) return;
	const float ig = rsqrt_nr(gg);
	const f3 dl = mk3(s->a.p.view.light_pos[0] - pt.x, s->a.p.view.light_pos[1] - pt.y, s->a.p.view.light_pos[2] - pt.z);
	const float ll = VR_FMA(dl.z, dl.z, VR_FMA(dl.y, dl.y, dl.x * dl.x));
	const float il = rsqrt_nr(ll);
	const float dot = VR_FMA(gz, dl.z, VR_FMA(gy, dl.y, gx * dl.x));
	const float sd = ll > 0.0f ? __builtin_fminf(__builtin_fabsf((dot * ig) * il), 1.0f) : 0.0f;
	const float iv = rsqrt_nr(VR_FMA(dir.z, dir.z, VR_FMA(dir.y, dir.y, dir.x * dir.x)));
	const f3 h = mk3(VR_FMA(-dir.x, iv, dl.x * il), VR_FMA(-dir.y, iv, dl.y * il), VR_FMA(-dir.z, iv, dl.z * il));
	const float hh = VR_FMA(h.z, h.z, VR_FMA(h.y, h.y, h.x * h.x));
	float sp = __builtin_fminf(__builtin_fabsf((VR_FMA(gz, h.z, VR_FMA(gy, h.y, gx * h.x)) * ig) * rsqrt_nr(hh)), 1.0f);
	sp = (ll > 0.0f && hh > 0.0f) ? sp : 0.0f;
	for (uint32_t n = s->a.light_n; n != 0u; n--) sp = sp * sp;
	m_out = select_lanes_else(lit, VR_FMA(s->a.light_kd, sd, s->a.light_ka), 1.0f);
	spec_out = select_lanes(lit, (s->a.light_ks * sp) * cw);
}

// The reference's cue of a dense sample (GPURenderer4.cu:41-51 shade_texture; the composite's): the field a hundredth towards the light
// against the field here, scaled by light_kd — 0 where params.light_kd <= 0.01f.  Its constants through the laundered pointer.
template <int BPV, int ADDR, int LAYOUT, bool Q8>
__device__ __forceinline__ float tf2d_cue(const void *vol, const RayKernelArgs &ka, const uint32_t *lut, f3 p3, float xb, float yb, float zb, float raw) {
	const Tf2dSegment s = tf2d_segment();
	if (!(s->a.p.light_kd > 0.01f)) return 0.0f;                             // wave-uniform
	const f3 dl = mk3(s->a.p.view.light_pos[0] - p3.x, s->a.p.view.light_pos[1] - p3.y, s->a.p.view.light_pos[2] - p3.z);
	const float inv = rsqrt_nr(VR_FMA(dl.z, dl.z, VR_FMA(dl.y, dl.y, dl.x * dl.x)));
	const float qx = VR_FMA(dl.x * inv, s->a.lh_x, xb), qy = VR_FMA(dl.y * inv, s->a.lh_y, yb), qz = VR_FMA(dl.z * inv, s->a.lh_z, zb);
	const TriFetch<BPV, LAYOUT> lf = tri_issue<BPV, ADDR, LAYOUT>(vol, ka, lut, qx, qy, qz, true);
	const float raw_l = tri_resolve<BPV, LAYOUT, Q8>(lf, ka, qx, qy, qz);
	return (raw_l - raw) * s->a.kd_scaled;
}

// Per pixel: label_kernel's shape (vr_label.hip) — the ray of raymarch_kernel under clip_segment, leap_lane over this unit's ESL words, kBatch
// samples issued back to back before the first is consumed behind a sched_barrier, finished lanes composited with weight 0 — with the
// contract's classification in place of the lookup.
//
// A sample: raw, tb, i, w as the composite forms them; the gradient (tf2d_gradient) where somebody needs it; the row coordinate
// tg = fmed3(g * g_scale, 0, rows - 1), j = min((uint32_t) tg, rows - 2), wg = tg - j; per channel c_j = fma(w, T[j][i1] - T[j][i], T[j][i]),
// c_j1 likewise, c = fma(wg, c_j1 - c_j, c_j); and behind it what the composite does with c: the dense test, the cue or the Blinn-Phong term
// of THIS gradient (wave-uniform: a.light_on), shadow_factor (a.shadow_on), the accumulation, early termination.
//
// Exact shortcuts, per wave: (1) all corners of every counting lane below skip_below and (2) the sample's coordinate below tf_zero_below,
// both derived from the table's envelope: every row is zero there, so c is exactly 0.  (3) the gradient is not fetched where nothing reads
// it: no counting lane's entry is g-dependent (every row holds row 0's bits at i and i1, so c is row 0's lookup whatever wg is:
// fma(wg, 0, x) = x) and, in a lit frame, no counting lane is dense under row 0.  Lanes then classify with g = 0: j = 0, wg = 0.
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void tf2d_kernel(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ table_g, const uint32_t *__restrict__ esl_g,
                 const Tf2dArgs d, uint32_t *out) {
	typedef LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)> L;
	constexpr uint32_t kThreads = L::threads;
	constexpr bool kQ8 = SAMPLING == VR_SAMPLE_TRILINEAR_Q8;
	static_assert(SAMPLING != VR_SAMPLE_NEAREST, "a tf2d frame is defined on the interpolated field");
	// samples per batch: two, as in label_kernel — the gradient's three components are live beside the colour and the fetch slots.  One on
	// the index-arithmetic rows of 1-byte voxels (label_kernel's exception) and on the 64-bit-table rows of 2-byte voxels, which need 65-66
	// registers at two (DESIGN.md section 4.15 has the table)
#ifndef VR_TF2D_BATCH
	constexpr int kBatch = (BPV == 1 && ADDR == kAddrWide) || (BPV == 2 && ADDR == kAddrLut64) ? 1 : 2;
#else
	constexpr int kBatch = VR_TF2D_BATCH;
#endif
	__shared__ __attribute__((aligned(16))) uint32_t lut[L::words];
	__shared__ Tf2dTables lds;
	if constexpr (L::max_dim != 0) stage_brick_tables<BPV, ADDR, LAYOUT>(a, lut);
	{
		const uint32_t t = threadIdx.x;
		const f4 *tf4 = (const f4 *) table_g;
		const uint32_t entries = (d.rows < VR_TF2D_ROWS_MAX ? d.rows : VR_TF2D_ROWS_MAX) * VR_TF_SIZE;
		for (uint32_t i = t; i < entries; i += kThreads) lds.tf[i] = tf4[i];
		for (uint32_t i = t; i < VR_ESL_VOLUME_SIZE; i += kThreads) lds.esl[i] = esl_g[i];
		if (t < 4u) lds.g_dependent[t] = t == 0u ? d.g_dependent[0] : (t == 1u ? d.g_dependent[1] : (t == 2u ? d.g_dependent[2] : d.g_dependent[3]));
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
	float k = kx;
	bool live = alive, done = false;
	f4 acc;
	acc.x = acc.y = acc.z = acc.w = 0.0f;
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
			// (1): skip_cmp is 0; an envelope without leading zero entries comes with skip_mask 0 and skip_cmp 1: 0 != 1 always
			if (__builtin_amdgcn_ballot_w64(c && (corners & a.skip_mask) != a.skip_cmp) == 0ull)
				continue;
			const float xb = VR_FMA(ks[u], A.x, B.x), yb = VR_FMA(ks[u], A.y, B.y), zb = VR_FMA(ks[u], A.z, B.z);
			const float raw = tri_resolve<BPV, LAYOUT, kQ8>(f[u], a, xb, yb, zb);
			const float tb = __builtin_amdgcn_fmed3f(VR_FMA(raw, a.tf_scale, -0.5f), 0.0f, (float) (VR_TF_SIZE - 1));
			// (2)
			if (__builtin_amdgcn_ballot_w64(c && tb >= a.tf_zero_below) == 0ull)
				continue;
			const uint32_t i = (uint32_t) (int) tb;
			const uint32_t i1 = i + 1u < VR_TF_SIZE ? i + 1u : VR_TF_SIZE - 1u;
			const float w = filter_weight<kQ8>(__builtin_amdgcn_fractf(tb));
			const bool frame_lit = tf2d_segment()->a.light_on != 0u;             // wave-uniform
			// (3): who reads the gradient
			uint64_t need = __builtin_amdgcn_ballot_w64(c && ((lds.g_dependent[i >> 5] >> (i & 31u)) & 1u) != 0u);
			if (need == 0ull && frame_lit) {
				const float a0 = lds.tf[i].w;
				need = __builtin_amdgcn_ballot_w64(c && VR_FMA(w, lds.tf[i1].w - a0, a0) > 0.05f);
			}
			float gx = 0.0f, gy = 0.0f, gz = 0.0f;
			if (need != 0ull) tf2d_gradient<BPV, ADDR, LAYOUT, kQ8>(vol, a, lut, A, B, ks[u], gx, gy, gz);
			f4 col;
			{   // steps 2-4: the row from the gradient's length, the two rows' lookups, their blend
				const Tf2dSegment s = tf2d_segment();
				const float gg = VR_FMA(gz, gz, VR_FMA(gy, gy, gx * gx));
				const float g = gg > 0.0f ? gg * rsqrt_nr(gg) : 0.0f;
				const float tg = __builtin_amdgcn_fmed3f(g * s->d.g_scale, 0.0f, s->d.top);
				uint32_t j = (uint32_t) tg;
				j = j < s->d.last ? j : s->d.last;
				const float wg = tg - (float) j;
				const f4 *row = lds.tf + j * VR_TF_SIZE;
				const f4 p0 = row[i], p1 = row[i1];
				f4 cj;
				cj.x = VR_FMA(w, p1.x - p0.x, p0.x); cj.y = VR_FMA(w, p1.y - p0.y, p0.y);
				cj.z = VR_FMA(w, p1.z - p0.z, p0.z); cj.w = VR_FMA(w, p1.w - p0.w, p0.w);
				const f4 q0 = row[VR_TF_SIZE + i], q1 = row[VR_TF_SIZE + i1];
				f4 ck;
				ck.x = VR_FMA(w, q1.x - q0.x, q0.x); ck.y = VR_FMA(w, q1.y - q0.y, q0.y);
				ck.z = VR_FMA(w, q1.z - q0.z, q0.z); ck.w = VR_FMA(w, q1.w - q0.w, q0.w);
				col.x = VR_FMA(wg, ck.x - cj.x, cj.x); col.y = VR_FMA(wg, ck.y - cj.y, cj.y);
				col.z = VR_FMA(wg, ck.z - cj.z, cj.z); col.w = VR_FMA(wg, ck.w - cj.w, cj.w);
			}
			const uint64_t dense = __builtin_amdgcn_ballot_w64(c && col.w > 0.05f);
			if (dense != 0ull) {
				if (frame_lit) {                                                 // vr_hip_set_lighting: Blinn-Phong from the gradient above
					float m, spec;
					tf2d_blinn_phong(gx, gy, gz, origin, dir, ks[u], dense, col.w, m, spec);
					col.x = VR_FMA(col.x, m, spec); col.y = VR_FMA(col.y, m, spec); col.z = VR_FMA(col.z, m, spec);
				} else {                                                         // the reference's cue; 0 for lanes that are not shaded
					const float diffuse = select_lanes(dense, tf2d_cue<BPV, ADDR, LAYOUT, kQ8>(vol, a, lut, march_point<SAMPLING>(origin, dir, ks[u]), xb, yb, zb, raw));
					col.x += diffuse; col.y += diffuse; col.z += diffuse;
				}
				if (lit_frame_shadowed()) {                                      // vr_hip_set_shadow: the light grid of the 1-D classification
					const float sf = select_lanes_else(dense, shadow_factor(march_point<SAMPLING>(origin, dir, ks[u])), 1.0f);
					col.x *= sf; col.y *= sf; col.z *= sf;
				}
			}
			const float t = c ? 1.0f - acc.w : 0.0f;                             // finished lanes: weight 0
			acc.x = VR_FMA(col.x, t, acc.x); acc.y = VR_FMA(col.y, t, acc.y);
			acc.z = VR_FMA(col.z, t, acc.z); acc.w = VR_FMA(col.w, t, acc.w);
			done = done || (c && acc.w > threshold);                             // early ray termination (CPURenderer.cpp:35-36)
		}
		live = live && !done;
	}

	// -- write_color and the fused clear: a pixel without a sample has accumulated nothing and stores 0.  The output address is read again in
	// the kernel-argument segment here, behind the march, instead of kept across it
	const uint32_t rgba = map_float_int(acc.x, 256) | (map_float_int(acc.y, 256) << 8) | (map_float_int(acc.z, 256) << 16) | (map_float_int(acc.w, 256) << 24);
	tf2d_segment()->out[px] = rgba;
}

hipError_t launch_tf2d(const RayKernelArgs &args, const Tf2dArgs &d, const void *linear, const void *bricked, uint32_t bpv,
                       const float *table, const uint32_t *esl_bits, void *out_rgba, hipStream_t stream) {
	if (table == nullptr || esl_bits == nullptr || out_rgba == nullptr || (args.shadow_on && args.shadow_q == 0ull) ||
	    args.p.sampling == VR_SAMPLE_NEAREST || d.rows < 2u || d.rows > VR_TF2D_ROWS_MAX || d.last != d.rows - 2u)
		return hipErrorInvalidValue;
	// the interpolated field from the copies a MIP frame reads: never NEAREST (refused above), the run bricks or the voxel bricks
	return launch_tiles<rows_field>(args, linear, bricked, bpv, stream, NoDynamicLds(),
	                                [&](auto row) { return VR_ROW_KERNEL(tf2d_kernel, row); },
	                                table, esl_bits, d, (uint32_t *) out_rgba);
}

// ---- the histogram over (value bin, gradient-magnitude row) ----

struct GradientHistogramArgs {
	uint32_t dim_x, dim_y, dim_z;
	uint32_t lines;                    // dim_y * dim_z
	float    half_x, half_y, half_z;
	float    g_scale, top;             // top = (float) (g_bins - 1)
	uint32_t counters;                 // g_bins * 256
};

// One workgroup per line of the linear array at a time (line = z * dim_y + y, grid-stride: every line, and so every voxel, is visited by
// exactly one workgroup whatever the grid is), one thread per voxel of the line at a time.  Six neighbour loads with indices clamped to
// their axis — the x neighbours lie in the same line —, and the voxel itself for the bin.  The gradient is step 2 of the tf2d contract at
// integer texel coordinates; row = (uint32_t) (fmed3(g * g_scale, 0, g_bins - 1) + 0.5f) <= g_bins - 1.  Each workgroup counts in LDS
// (32-bit counters: the launcher bounds the voxels per workgroup) and adds its non-zero counters to the 64-bit ones in memory.
template <int BPV>
__global__ __launch_bounds__(256)
void gradient_histogram_kernel(const void *__restrict__ vol, const GradientHistogramArgs h, unsigned long long *__restrict__ hist
#ifdef VR_BOUNDS_CHECK
                               , const RayKernelArgs bc
#endif
                               ) {
	typedef typename VoxelT<BPV>::type V;
	__shared__ uint32_t sh[VR_GRADIENT_BINS_MAX * 256];
	for (uint32_t i = threadIdx.x; i < h.counters; i += 256u) sh[i] = 0u;
	__syncthreads();
	const V *v = (const V *) vol;
#ifdef VR_BOUNDS_CHECK
	auto at = [&](uint64_t idx) -> float { return (float) *VR_BC_POINTER(bc, const V *, v + idx, (uint32_t) sizeof(V)); };
#else
	auto at = [&](uint64_t idx) -> float { return (float) v[idx]; };
#endif
	for (uint32_t line = blockIdx.x; line < h.lines; line += gridDim.x) {
		const uint32_t z = line / h.dim_y, y = line - z * h.dim_y;
		const uint32_t ym = y > 0u ? y - 1u : 0u, yp = y + 1u < h.dim_y ? y + 1u : y;
		const uint32_t zm = z > 0u ? z - 1u : 0u, zp = z + 1u < h.dim_z ? z + 1u : z;
		const uint64_t base = (uint64_t) line * h.dim_x;
		const uint64_t base_ym = ((uint64_t) z * h.dim_y + ym) * h.dim_x, base_yp = ((uint64_t) z * h.dim_y + yp) * h.dim_x;
		const uint64_t base_zm = ((uint64_t) zm * h.dim_y + y) * h.dim_x, base_zp = ((uint64_t) zp * h.dim_y + y) * h.dim_x;
		for (uint32_t x = threadIdx.x; x < h.dim_x; x += 256u) {
			const uint32_t xm = x > 0u ? x - 1u : 0u, xp = x + 1u < h.dim_x ? x + 1u : x;
			const float centre = at(base + x);
			const float gx = (at(base + xp) - at(base + xm)) * h.half_x;
			const float gy = (at(base_yp + x) - at(base_ym + x)) * h.half_y;
			const float gz = (at(base_zp + x) - at(base_zm + x)) * h.half_z;
			const float gg = VR_FMA(gz, gz, VR_FMA(gy, gy, gx * gx));
			const float g = gg > 0.0f ? gg * rsqrt_nr(gg) : 0.0f;
			const float tg = __builtin_amdgcn_fmed3f(g * h.g_scale, 0.0f, h.top);
			const uint32_t row = (uint32_t) (tg + 0.5f);
			const uint32_t raw = (uint32_t) centre;
			const uint32_t bin = BPV == 1 ? raw : raw >> 8;
			uint32_t slot = row * 256u + bin;
			slot = slot < h.counters ? slot : h.counters - 1u;                   // (never binding: row <= g_bins - 1, bin <= 255)
			atomicAdd(&sh[slot], 1u);
		}
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < h.counters; i += 256u) {
		const uint32_t n = sh[i];
		if (n != 0u) atomicAdd(&hist[i], (unsigned long long) n);
	}
}

hipError_t launch_gradient_histogram(const void *volume, uint32_t bpv, const uint32_t dims[3], uint32_t g_bins, float g_scale,
                                     unsigned long long *hist, const RayKernelArgs *bc, hipStream_t stream) {
	if (volume == nullptr || hist == nullptr || g_bins < 1u || g_bins > VR_GRADIENT_BINS_MAX || dims[0] == 0u || dims[1] == 0u || dims[2] == 0u)
		return hipErrorInvalidValue;
	const uint64_t lines = (uint64_t) dims[1] * dims[2];
	if (lines > 0xffffffffull) return hipErrorInvalidValue;
	hipError_t e = hipMemsetAsync(hist, 0, (size_t) g_bins * 256u * sizeof(unsigned long long), stream);
	if (e != hipSuccess) return e;
	GradientHistogramArgs h;
	h.dim_x = dims[0]; h.dim_y = dims[1]; h.dim_z = dims[2]; h.lines = (uint32_t) lines;
	h.half_x = 0.5f * (float) dims[0]; h.half_y = 0.5f * (float) dims[1]; h.half_z = 0.5f * (float) dims[2];
	h.g_scale = g_scale; h.top = (float) (g_bins - 1u); h.counters = g_bins * 256u;
	// the grid from the voxel count: a workgroup per 4096 voxels, at least one, at most 8192 and never more than there are lines; a line
	// holds at most 65535 voxels, so a workgroup's share of lines stays below 2^32 voxels once the grid has lines / 65536 workgroups
	const uint64_t voxels = lines * dims[0];
	uint64_t blocks = (voxels + 4095u) / 4096u;
	if (blocks > 8192u) blocks = 8192u;
	if (blocks < (lines >> 16) + 1u) blocks = (lines >> 16) + 1u;
	if (blocks > lines) blocks = lines;
#ifdef VR_BOUNDS_CHECK
	if (bc == nullptr) return hipErrorInvalidValue;
	if (bpv == 1) hipLaunchKernelGGL(gradient_histogram_kernel<1>, dim3((uint32_t) blocks), dim3(256), 0, stream, volume, h, hist, *bc);
	else          hipLaunchKernelGGL(gradient_histogram_kernel<2>, dim3((uint32_t) blocks), dim3(256), 0, stream, volume, h, hist, *bc);
#else
	(void) bc;
	if (bpv == 1) hipLaunchKernelGGL(gradient_histogram_kernel<1>, dim3((uint32_t) blocks), dim3(256), 0, stream, volume, h, hist);
	else          hipLaunchKernelGGL(gradient_histogram_kernel<2>, dim3((uint32_t) blocks), dim3(256), 0, stream, volume, h, hist);
#endif
	return hipGetLastError();
}

}  // namespace vr
