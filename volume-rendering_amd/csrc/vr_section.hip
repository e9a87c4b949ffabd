// vr_section.hip — section frames (vr_hip_render_section): the oblique slice through the interpolated field and its
// thick-slab forms (slab MIP, slab MinIP, slab mean), coloured by the transfer function or a grey window, with the depth layer a backdrop
// frame takes.  One kernel family, section_kernel, over the 24 rows of the isosurface, and its launcher.
#include "vr_march.h"

namespace vr {

// Per pixel: the ray of raymarch_kernel (get_ray, intersect) under clip_segment (the identity clip when none is set), the parameter kc at
// which it crosses the section plane — the clip plane's two expressions dn and on, from the unreplaced direction, kc = -on / dn —, and the
// segment narrowed to the slab |n . x + d| <= h: [kc, kc] for a POINT frame, [max(kx, min(ka, kb)), min(ky, max(ka, kb))] for the thick modes.
// On that segment the sample sequence of mip_kernel's TRILINEAR march without skipping: k starts at kx, advances by repeated addition of
// ray_step, every position is fma(k, A, B).  kBatch samples are issued back to back before the first is consumed behind a sched_barrier, in
// sample order: the sum of a MEAN frame adds in that order.  A finished lane stops ON its last sample and fetches it again (every fetch
// clamps its cell: the address is in bounds whatever k is): the value it resolves is one it has counted, so maximum and minimum need no
// test of liveness, and sum and count take 0 from it.
//
// The mode is a wave-uniform kernel argument, not a template parameter: every sample updates the maximum, the minimum, the sum and the count
// (a max, a min, two selects and two adds beside a trilinear sample's ~100 VALU operations), the pixel's value is chosen after the loop.
// POINT is the same march on [kc, kc]: one sample, of which maximum, minimum and mean are all the value.
//
// The colour is the filtered transfer-function lookup of a MIP pixel, or with a window the opaque grey fmed3((value - lo) * inv, 0, 1);
// depth (where the caller gave a buffer) is kc or the narrowed kx, -1 for every pixel without a section.
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void section_kernel(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g, const SectionArgs s,
                    uint32_t *__restrict__ out, float *__restrict__ depth) {
	typedef LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)> L;
	constexpr uint32_t kThreads = L::threads;
	constexpr bool kQ8 = SAMPLING == VR_SAMPLE_TRILINEAR_Q8;
	static_assert(SAMPLING != VR_SAMPLE_NEAREST, "a section is defined on the interpolated field");
	// samples per batch: those of the mip_clipped kernel of the same row (vr_mip_body.inc), whose registers this kernel is held to
	constexpr int kBatch = BPV == 1 && ADDR == kAddrWide && LAYOUT == kLayoutBricked ? 3 : 4;
	__shared__ __attribute__((aligned(16))) uint32_t lut[L::words];
	if constexpr (L::max_dim != 0) stage_brick_tables<BPV, ADDR, LAYOUT>(a, lut);
	__syncthreads();

	// -- tile = workgroup id: every ray of a section frame is a full march of its slab
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

	// -- the section plane and the slab around it: the segment becomes the slab's part of it
	const float dn = VR_FMA(s.plane[2], dir.z, VR_FMA(s.plane[1], dir.y, s.plane[0] * dir.x));
	const float on = VR_FMA(s.plane[2], origin.z, VR_FMA(s.plane[1], origin.y, VR_FMA(s.plane[0], origin.x, s.plane[3])));
	const bool point = s.mode == VR_SECTION_POINT;      // wave-uniform: a kernel argument
	float front;
	if (point) {
		const float kc = -on / dn;
		alive = alive && dn != 0 && (kx <= kc) && (kc <= ky);
		kx = kc; ky = kc;
		front = kc;
	} else {
		const float ka = ((-s.half_width) - on) / dn, kb = (s.half_width - on) / dn;
		kx = flmax(kx, flmin(ka, kb));
		ky = flmin(ky, flmax(ka, kb));
		alive = alive && dn != 0 && (kx < ky) && (ky > 0);
		front = kx;
	}
	const bool hit = alive;
	if (!alive) { kx = 0.0f; ky = 0.0f; origin = mk3(0.0f, 0.0f, 0.0f); dir = origin; }      // lanes without a section: position 0, never live

	// -- the march: mip_kernel's batch without skipping; maximum, minimum, sum and count of the samples that count
	const f3 A = mk3(dir.x * a.half_x, dir.y * a.half_y, dir.z * a.half_z);
	const f3 B = mk3(VR_FMA(origin.x, a.half_x, a.off_x), VR_FMA(origin.y, a.half_y, a.off_y), VR_FMA(origin.z, a.half_z, a.off_z));
	float k = kx;
	bool live = alive;
	float vmax = 0.0f, vmin = __builtin_inff(), sum = 0.0f;
	uint32_t n = 0u;
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
			const float raw = tri_resolve<BPV, LAYOUT, kQ8>(f[u], a, VR_FMA(ks[u], A.x, B.x), VR_FMA(ks[u], A.y, B.y), VR_FMA(ks[u], A.z, B.z));
			vmax = __builtin_fmaxf(vmax, raw);      // (raw is never NaN, and a sample that does not count repeats one that did)
			vmin = __builtin_fminf(vmin, raw);
			sum = sum + (counts[u] ? raw : 0.0f);   // (sum + 0 is sum, exactly)
			n += counts[u] ? 1u : 0u;
		}
	}

	// -- the value of the mode, its colour (write_color of the entry as stored, or of the grey), the fused clear: misses store 0 and -1
	uint32_t rgba = 0;
	if (hit) {
		float value = vmax;                         // VR_SECTION_MAX, and the one sample of VR_SECTION_POINT
		if (s.mode == VR_SECTION_MIN) value = vmin;
		else if (s.mode == VR_SECTION_MEAN) value = sum / (float) n;
		f4 colour;
		if (s.windowed) {
			const float g = __builtin_amdgcn_fmed3f((value - s.window_lo) * s.window_inv, 0.0f, 1.0f);
			colour.x = colour.y = colour.z = g; colour.w = 1.0f;
		} else {
			// the filtered lookup of a MIP pixel (vr_mip_body.inc): entries floor(tb) and floor(tb) + 1, clamp addressing
			const f4 *tf4 = (const f4 *) tf_g;
			const float tb = __builtin_amdgcn_fmed3f(VR_FMA(value, a.tf_scale, -0.5f), 0.0f, (float) (VR_TF_SIZE - 1));
			const uint32_t i = (uint32_t) (int) tb, i1 = i + 1u < VR_TF_SIZE ? i + 1u : i;
			const float w = filter_weight<kQ8>(__builtin_amdgcn_fractf(tb));
			const f4 c0 = tf4[i], c1 = tf4[i1];
			colour.x = VR_FMA(w, c1.x - c0.x, c0.x); colour.y = VR_FMA(w, c1.y - c0.y, c0.y);
			colour.z = VR_FMA(w, c1.z - c0.z, c0.z); colour.w = VR_FMA(w, c1.w - c0.w, c0.w);
		}
		rgba = map_float_int(colour.x, 256) | (map_float_int(colour.y, 256) << 8) |
		       (map_float_int(colour.z, 256) << 16) | (map_float_int(colour.w, 256) << 24);
	}
	out[px] = rgba;
	if (depth != nullptr) depth[px] = hit ? front : -1.0f;       // (wave-uniform: a kernel argument)
}

hipError_t launch_section(const RayKernelArgs &args, const SectionArgs &section, const void *linear, const void *bricked, uint32_t bpv,
                          const float *tf, void *out_rgba, void *out_depth, hipStream_t stream) {
	if (section.mode > VR_SECTION_MEAN) return hipErrorInvalidValue;
	// the interpolated field from the copies a MIP frame reads: never NEAREST (the caller refuses it), the run bricks or the voxel bricks
	return launch_tiles<rows_field>(args, linear, bricked, bpv, stream, NoDynamicLds(),
	                                [&](auto row) { return VR_ROW_KERNEL(section_kernel, row); },
	                                tf, section, (uint32_t *) out_rgba, (float *) out_depth);
}

}  // namespace vr
