// vr_label.hip — labelled composite frames (vr_hip_render_labelled): the composite frame of a TRILINEAR view with a second,
// 1-byte volume of segment labels whose per-label table entry tints, replaces or hides what the transfer function returns for a sample.  One
// kernel family, label_kernel, over the 24 rows of the isosurface, and its launcher.
#include "vr_march.h"

namespace vr {

// LDS beside the brick tables: the premultiplied transfer function and its per-entry deltas (the same fp32 subtraction the composite's dtf
// holds), the ESL bits, and the label table as { colour, mix } and opacity: one 16-byte and one 4-byte read per labelled sample.  13 KiB;
// with the 50 KiB of the 64-bit address tables a CU still holds the two workgroups of the row's depth_kernel twin, so nothing is packed.
struct __attribute__((aligned(16))) LabelTables {
	f4 tf[VR_TF_SIZE], dtf[VR_TF_SIZE];
	f4 tint[VR_LABEL_COUNT];           // colour[0..2], mix
	float opacity[VR_LABEL_COUNT];
	uint32_t esl[VR_ESL_VOLUME_SIZE];
};

// the kernel-argument segment of label_kernel as a struct: its arguments in order
struct LabelKernelSegment { RayKernelArgs a; const void *vol; const float *tf; const uint32_t *esl; LabelArgs d; const float *table; uint32_t *out; };

// wave-uniform words of the frame, read where they are used through the laundered kernel-argument pointer (vr_march.h clip_segment)
// (-DVR_LABEL_LIT=0 / 1 makes it a constant: what a second, lit family would compile to — the register figures of DESIGN.md section 4.14)
__device__ __forceinline__ bool label_frame_lit() {
#ifdef VR_LABEL_LIT
	return VR_LABEL_LIT != 0;
#endif
	typedef const RayKernelArgs __attribute__((address_space(4))) *ConstArgs;
	ConstArgs a = (ConstArgs) __builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(a));
	return a->light_on != 0u;
}

// Step 1 of the contract: the label of the voxel nearest to the texel coordinates (xb, yb, zb) — the index per axis is
// (uint32_t) fmed3(x + 0.5f, 0, N - 1), the add one plain IEEE add (the units are compiled with -ffp-contract=off) —, one vector byte load.
// Where the label copy follows the field's quad bricks (d.bricked, wave-uniform: 1-byte voxels behind address tables, chunk plane (x,y)) the
// byte's offset is the staged tables' element offset: their byte offsets shifted right by the element size, 4 bytes.  Otherwise it is the index
// into the linear array.  In bounds for every lane whatever the coordinates are: every index is clamped to its axis.
template <int BPV, int ADDR, int LAYOUT>
__device__ __forceinline__ uint32_t fetch_label(const RayKernelArgs &ka, const uint32_t *lut, float xb, float yb, float zb) {
	// the label array, its order and the volume's dims are read HERE through the laundered kernel-argument pointer (vr_march.h clip_segment):
	// nothing of them occupies a scalar register across the march
	typedef const LabelKernelSegment __attribute__((address_space(4))) *ConstSegment;
	ConstSegment s = (ConstSegment) __builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(s));
	uint32_t ix = (uint32_t) __builtin_amdgcn_fmed3f(xb + 0.5f, 0.0f, s->a.max_x);
	uint32_t iy = (uint32_t) __builtin_amdgcn_fmed3f(yb + 0.5f, 0.0f, s->a.max_y);
	uint32_t iz = (uint32_t) __builtin_amdgcn_fmed3f(zb + 0.5f, 0.0f, s->a.max_z);
	constexpr bool kTables = BPV == 1 && LAYOUT == kLayoutBricked && ADDR != kAddrWide;
	const uint8_t *base = (const uint8_t *) (uintptr_t) s->d.labels, *q;
	if (kTables && s->d.bricked != 0u) {
		typedef LutCfg<ADDR> L;
		ix = (uint32_t) VR_BC_INDEX(ka, 0, (int) ix); iy = (uint32_t) VR_BC_INDEX(ka, 1, (int) iy); iz = (uint32_t) VR_BC_INDEX(ka, 2, (int) iz);
		const uint32_t exy = lut[L::x_at + kLutPad + ix] + lut[L::y_at + kLutPad + iy];
		if (ADDR == kAddr32) q = base + ((exy + lut[L::z_words * (iz + kLutPad)]) >> 2);
		else {
			const uint2 z = *(const uint2 *) (lut + L::z_words * (iz + kLutPad));
			q = base + (((((uint64_t) z.y) << 32 | z.x) + exy) >> 2);
		}
	} else if (ADDR == kAddr32) {
		q = base + ((iz * s->a.dim_y + iy) * s->a.dim_x + ix);
	} else {
		q = base + (((uint64_t) iz * s->a.dim_y + iy) * s->a.dim_x + ix);
	}
	return *VR_BC_POINTER(ka, const uint8_t *, q, 1u);
}

// The reference's cue of a dense sample (GPURenderer4.cu:41-51 shade_texture; the composite's, vr_raymarch_body.inc): the field a hundredth
// towards the light against the field here, scaled by light_kd — 0 where params.light_kd <= 0.01f.  Its constants through the laundered pointer.
template <int BPV, int ADDR, int LAYOUT, bool Q8>
__device__ __forceinline__ float label_cue(const void *vol, const RayKernelArgs &ka, const uint32_t *lut, f3 p3, float xb, float yb, float zb, float raw) {
	typedef const RayKernelArgs __attribute__((address_space(4))) *ConstArgs;
	ConstArgs a = (ConstArgs) __builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(a));
	if (!(a->p.light_kd > 0.01f)) return 0.0f;                               // wave-uniform
	const f3 dl = mk3(a->p.view.light_pos[0] - p3.x, a->p.view.light_pos[1] - p3.y, a->p.view.light_pos[2] - p3.z);
	const float inv = rsqrt_nr(VR_FMA(dl.z, dl.z, VR_FMA(dl.y, dl.y, dl.x * dl.x)));
	const float qx = VR_FMA(dl.x * inv, a->lh_x, xb), qy = VR_FMA(dl.y * inv, a->lh_y, yb), qz = VR_FMA(dl.z * inv, a->lh_z, zb);
	const TriFetch<BPV, LAYOUT> lf = tri_issue<BPV, ADDR, LAYOUT>(vol, ka, lut, qx, qy, qz, true);
	const float raw_l = tri_resolve<BPV, LAYOUT, Q8>(lf, ka, qx, qy, qz);
	return (raw_l - raw) * a->kd_scaled;
}

// Per pixel: the ray of raymarch_kernel (get_ray, intersect) under clip_segment (the identity clip when none is set), the composite's leaping
// loop in its plain per-lane form (vr_march.h leap_lane), and on what is left the composite's sample sequence — k starts at the leapt kx, advances by repeated
// addition of ray_step, every position is fma(k, A, B) — in the depth kernel's shape: kBatch samples are issued back to back before the first
// is consumed behind a sched_barrier, in sample order.  A lane that is finished — beyond ky, or terminated by acc.w > ray_threshold inside a
// batch already issued — stays ON its last sample and fetches it again (every fetch clamps its cell: in bounds whatever k is); it is composited
// with weight 0: fma(c, 0, acc) is acc for the finite c of a lookup.
//
// A sample: the filtered lookup c at tb, then the label (fetch_label, and the table entry e: c.xyz = fma(e.mix, fma(e.colour, c.w, -c.xyz), c.xyz)
// with the unscaled c.w, then all four channels times e.opacity), and behind it what the composite does with c: the dense test, the cue or
// light_sample (wave-uniform: a.light_on), shadow_factor (a.shadow_on), the accumulation, early termination.
//
// Exact shortcuts, per wave: (1) all corners of every counting lane below skip_below — the sample is transparent, nothing is unpacked and no
// label is fetched; (2) the sample's coordinate below tf_zero_below: c is exactly 0 and stays 0 under any entry.  The label of a sample that
// passes both is one dependent byte load (VR_LABEL_EARLY: issued with the batch for every sample instead; DESIGN.md section 4.14 has the
// figures of both forms).
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void label_kernel(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g, const uint32_t *__restrict__ esl_g,
                  const LabelArgs d, const float *__restrict__ table_g, uint32_t *out) {
	typedef LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)> L;
	constexpr uint32_t kThreads = L::threads;
	constexpr bool kQ8 = SAMPLING == VR_SAMPLE_TRILINEAR_Q8;
	static_assert(SAMPLING != VR_SAMPLE_NEAREST, "a labelled frame is defined on the interpolated field");
	// samples per batch: two, against the depth kernel's four — colour, the ray's origin and direction (the cue, the lighting and the shadow need
	// the model-space point) and the label are live beside the fetch slots, and at three a SIMD holds 7 waves, at four 5-6 (DESIGN.md section
	// 4.14 has the table).  One on the index-arithmetic rows of 1-byte voxels, whose 64-bit address chains cost another 6-9 registers.
#ifndef VR_LABEL_BATCH
	constexpr int kBatch = BPV == 1 && ADDR == kAddrWide ? 1 : 2;
#else
	constexpr int kBatch = VR_LABEL_BATCH;
#endif
	__shared__ __attribute__((aligned(16))) uint32_t lut[L::words];
	__shared__ LabelTables lds;
	if constexpr (L::max_dim != 0) stage_brick_tables<BPV, ADDR, LAYOUT>(a, lut);
	{
		const uint32_t t = threadIdx.x;
		if (t < VR_TF_SIZE) {
			const f4 *tf4 = (const f4 *) tf_g;
			const uint32_t t1 = t + 1 < VR_TF_SIZE ? t + 1 : VR_TF_SIZE - 1;
			const f4 c0 = tf4[t], c1 = tf4[t1];
			f4 dc;
			dc.x = c1.x - c0.x; dc.y = c1.y - c0.y; dc.z = c1.z - c0.z; dc.w = c1.w - c0.w;
			lds.tf[t] = c0;
			lds.dtf[t] = dc;
		}
		if (t < VR_LABEL_COUNT) {
			const float *e = table_g + 5u * t;
			f4 tint;
			tint.x = e[0]; tint.y = e[1]; tint.z = e[2]; tint.w = e[3];
			lds.tint[t] = tint;
			lds.opacity[t] = e[4];
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
	float k = kx;
	bool live = alive, done = false;
	f4 acc;
	acc.x = acc.y = acc.z = acc.w = 0.0f;
	while (__builtin_amdgcn_ballot_w64(live) != 0ull) {
		TriFetch<BPV, LAYOUT> f[kBatch];
		float ks[kBatch];
		bool counts[kBatch];
#ifdef VR_LABEL_EARLY
		uint32_t early[kBatch];
#endif
		#pragma unroll
		for (int u = 0; u < kBatch; u++) {
			ks[u] = k;
			counts[u] = live;
			f[u] = tri_issue<BPV, ADDR, LAYOUT>(vol, a, lut, VR_FMA(k, A.x, B.x), VR_FMA(k, A.y, B.y), VR_FMA(k, A.z, B.z), true);
#ifdef VR_LABEL_EARLY
			early[u] = fetch_label<BPV, ADDR, LAYOUT>(a, lut, VR_FMA(k, A.x, B.x), VR_FMA(k, A.y, B.y), VR_FMA(k, A.z, B.z));
#endif
			const float next = k + step;            // (a lane whose next sample lies beyond ky stays ON its last sample)
			live = live && next <= ky;
			k = live ? next : k;
		}
		__builtin_amdgcn_sched_barrier(0);
		#pragma unroll
		for (int u = 0; u < kBatch; u++) {
			const bool c = counts[u] && !done;
			const uint32_t corners = f[u].w0 | f[u].w1 | f[u].w2 | f[u].w3;     // (words a layout does not fetch are 0)
			// (1): skip_cmp is 0; a transfer function without leading zero entries comes with skip_mask 0 and skip_cmp 1: 0 != 1 always
			if (__builtin_amdgcn_ballot_w64(c && (corners & a.skip_mask) != a.skip_cmp) == 0ull)
				continue;
			const float xb = VR_FMA(ks[u], A.x, B.x), yb = VR_FMA(ks[u], A.y, B.y), zb = VR_FMA(ks[u], A.z, B.z);
			const float raw = tri_resolve<BPV, LAYOUT, kQ8>(f[u], a, xb, yb, zb);
			const float tb = __builtin_amdgcn_fmed3f(VR_FMA(raw, a.tf_scale, -0.5f), 0.0f, (float) (VR_TF_SIZE - 1));
			// (2)
			if (__builtin_amdgcn_ballot_w64(c && tb >= a.tf_zero_below) == 0ull)
				continue;
#ifdef VR_LABEL_EARLY
			const uint32_t l = early[u];
#else
			const uint32_t l = fetch_label<BPV, ADDR, LAYOUT>(a, lut, xb, yb, zb);
#endif
			f4 col;
			{
				const uint32_t i = (uint32_t) (int) tb;
				const float w = filter_weight<kQ8>(__builtin_amdgcn_fractf(tb));
				const f4 c0 = lds.tf[i], dc = lds.dtf[i];
				col.x = VR_FMA(w, dc.x, c0.x); col.y = VR_FMA(w, dc.y, c0.y);
				col.z = VR_FMA(w, dc.z, c0.z); col.w = VR_FMA(w, dc.w, c0.w);
			}
			{   // the insertion: the table entry of the sample's label
				const f4 e = lds.tint[l & (VR_LABEL_COUNT - 1u)];
				const float op = lds.opacity[l & (VR_LABEL_COUNT - 1u)];
				col.x = VR_FMA(e.w, VR_FMA(e.x, col.w, -col.x), col.x);
				col.y = VR_FMA(e.w, VR_FMA(e.y, col.w, -col.y), col.y);
				col.z = VR_FMA(e.w, VR_FMA(e.z, col.w, -col.z), col.z);
				col.x = col.x * op; col.y = col.y * op; col.z = col.z * op; col.w = col.w * op;
			}
			const uint64_t dense = __builtin_amdgcn_ballot_w64(c && col.w > 0.05f);
			if (dense != 0ull) {
				if (label_frame_lit()) {                                         // vr_hip_set_lighting: Blinn-Phong from the field's gradient
					float m, spec;
					light_sample<BPV, ADDR, LAYOUT, kQ8>(vol, a, lut, A, B, origin, dir, ks[u], dense, col.w, m, spec);
					col.x = VR_FMA(col.x, m, spec); col.y = VR_FMA(col.y, m, spec); col.z = VR_FMA(col.z, m, spec);
				} else {                                                         // the reference's cue; 0 for lanes that are not shaded
					const float diffuse = select_lanes(dense, label_cue<BPV, ADDR, LAYOUT, kQ8>(vol, a, lut, march_point<SAMPLING>(origin, dir, ks[u]), xb, yb, zb, raw));
					col.x += diffuse; col.y += diffuse; col.z += diffuse;
				}
				if (lit_frame_shadowed()) {                                      // vr_hip_set_shadow: the light grid of the unlabelled classification
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

	// -- RaycasterBase.h:44-50 write_color and the fused clear: a pixel without a sample has accumulated nothing and stores 0.  The output address
	// is read again in the kernel-argument segment here, behind the march, instead of kept across it
	const uint32_t rgba = map_float_int(acc.x, 256) | (map_float_int(acc.y, 256) << 8) | (map_float_int(acc.z, 256) << 16) | (map_float_int(acc.w, 256) << 24);
	typedef const LabelKernelSegment __attribute__((address_space(4))) *ConstSegment;
	ConstSegment seg = (ConstSegment) __builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(seg));
	seg->out[px] = rgba;
}

hipError_t launch_labelled(const RayKernelArgs &args, const void *labels_linear, const void *labels_xy_bricks, const void *linear, const void *bricked,
                           uint32_t bpv, const float *tf, const uint32_t *esl_bits, const float *table, void *out_rgba, hipStream_t stream) {
	if (labels_linear == nullptr || table == nullptr || esl_bits == nullptr || out_rgba == nullptr || (args.shadow_on && args.shadow_q == 0ull) ||
	    args.p.sampling == VR_SAMPLE_NEAREST)
		return hipErrorInvalidValue;
	// the label bricks where the row that will run stages the tables of the (x,y) quad copy of 1-byte voxels (fetch_label kTables)
	const bool tables = labels_xy_bricks != nullptr && args.brick_plane == kPlaneXY &&
		select_variant(args, bricked != nullptr, bpv, [](auto, auto voxel, auto addr, auto layout, bool) {
			return decltype(voxel)::value == 1 && decltype(layout)::value == (int) kLayoutBricked && decltype(addr)::value != (int) kAddrWide; });
	LabelArgs labels;
	labels.labels = (uint64_t) (uintptr_t) (tables ? labels_xy_bricks : labels_linear);
	labels.bricked = tables ? 1u : 0u;
	labels.reserved = 0u;
	RayKernelArgs a = args;
#ifdef VR_BOUNDS_CHECK
	// the label array is the second array the checks accept (bc_address): the rows of this family read no other alternate copy
	a.alt_copy = labels.labels;
	a.bc_alt_bytes = tables ? bricked_elems(a.dim_x, a.dim_y, a.dim_z) : (uint64_t) a.dim_x * a.dim_y * a.dim_z;
#endif
	// the interpolated field from the copies a MIP frame reads: never NEAREST (refused above), the run bricks or the voxel bricks
	return launch_tiles<rows_field>(a, linear, bricked, bpv, stream, NoDynamicLds(),
	                                [&](auto row) { return VR_ROW_KERNEL(label_kernel, row); },
	                                tf, esl_bits, labels, table, (uint32_t *) out_rgba);
}

}  // namespace vr
