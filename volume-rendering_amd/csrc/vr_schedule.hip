// vr_schedule.hip — the launch order of a frame's tiles: tile_order_kernel (measured cost), tile_estimate_kernel (first frame),
// tile_choice_kernel (which run copy per block of tiles), and their launchers.
#include "vr_march.h"

namespace vr {

// ---- measured-cost tile order -------------------------------------------------------------------------------------------------
//
// The hardware starts workgroups in id order as slots free up; rays of very different length (empty-space leaping, early
// termination, rays that probe along a block face) make some tiles 10-50x longer than others, and a long tile that starts late
// IS the tail of the frame.  A frame can record what every tile cost (tile_cost: the longest wave of the tile, in 64-cycle units);
// this kernel turns that into a launch order for the next frame with the same parameters: tiles binned by cost into kOrderBins
// bins, most expensive bin first, original tile order inside a bin (neighbouring tiles of similar cost stay neighbours: they share
// cache lines).  One workgroup, a stable counting sort through LDS; clears the costs for the next recording.  Placement only.
#ifndef VR_ORDER_BINS
#define VR_ORDER_BINS 16
#endif
constexpr uint32_t kOrderBins = VR_ORDER_BINS, kOrderThreads = 512;

__global__ __launch_bounds__(kOrderThreads)
void tile_order_kernel(uint32_t *__restrict__ cost, uint32_t *__restrict__ order, uint32_t ntiles) {
	__shared__ uint32_t wave_total[kOrderBins][kOrderThreads / 64u], bin_total[kOrderBins];
	__shared__ uint32_t vmax;
	// up to kOrderCached tiles (a 2048^2 frame has 8192) the costs are read ONCE, coalesced, into LDS and the three passes below run on that
	// copy (each thread owns a contiguous run of tiles, i.e. strided global reads otherwise); larger frames read them from memory
	constexpr uint32_t kOrderCached = 8192;
	__shared__ uint32_t cached[kOrderCached];
	const uint32_t t = threadIdx.x;
	const uint32_t chunk = (ntiles + kOrderThreads - 1) / kOrderThreads, lo = t * chunk < ntiles ? t * chunk : ntiles, hi = lo + chunk < ntiles ? lo + chunk : ntiles;
	const bool in_lds = ntiles <= kOrderCached;
	if (in_lds) for (uint32_t i = t; i < ntiles; i += kOrderThreads) { cached[i] = cost[i]; cost[i] = 0; }      // (cleared for the next recording on the way)
	if (t == 0) vmax = 0;
	__syncthreads();
	auto cost_of = [&](uint32_t i) { return in_lds ? cached[i] : cost[i]; };
	uint32_t m = 0;
	for (uint32_t i = lo; i < hi; i++) { const uint32_t c = cost_of(i); m = c > m ? c : m; }
	atomicMax(&vmax, m);
	__syncthreads();
	// (bins by a float product: the 64-bit division the first version used here, twice per tile, was most of the kernel's 25 us; any
	// monotone function does as long as both passes use the same one)
	const float scale = (float) kOrderBins / ((float) vmax + 1.0f);
	auto bin_of = [&](uint32_t c) { const uint32_t q = (uint32_t) ((float) c * scale); return kOrderBins - 1u - (q < kOrderBins ? q : kOrderBins - 1u); };    // 0 = most expensive
	uint32_t mine[kOrderBins];
	for (uint32_t b = 0; b < kOrderBins; b++) mine[b] = 0;
	for (uint32_t i = lo; i < hi; i++) mine[bin_of(cost_of(i))]++;
	// exclusive scan of every bin's per-thread counts over the 512 threads: inside a wave by shuffles, across the 8 waves through LDS
	// (the first version scanned each bin serially in one thread: 22 of the kernel's 26 us)
	const uint32_t lane = t & 63u, wave = t >> 6;
	uint32_t before[kOrderBins];
	for (uint32_t b = 0; b < kOrderBins; b++) {
		uint32_t v = mine[b];
		#pragma unroll
		for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t n = __shfl_up(v, d, 64); if (lane >= d) v += n; }
		before[b] = v - mine[b];
		if (lane == 63u) wave_total[b][wave] = v;
	}
	__syncthreads();
	if (t < kOrderBins) {
		uint32_t run = 0;
		for (uint32_t w = 0; w < kOrderThreads / 64u; w++) { const uint32_t c = wave_total[t][w]; wave_total[t][w] = run; run += c; }
		bin_total[t] = run;
	}
	__syncthreads();
	uint32_t base = 0, pos[kOrderBins];
	for (uint32_t b = 0; b < kOrderBins; b++) { pos[b] = base + wave_total[b][wave] + before[b]; base += bin_total[b]; }
	for (uint32_t i = lo; i < hi; i++) { order[pos[bin_of(cost_of(i))]++] = i; }
	if (!in_lds) {
		__syncthreads();
		for (uint32_t i = lo; i < hi; i++) cost[i] = 0;
	}
}

// ---- a launch order for the FIRST frame of a policy key (round 4) ------------------------------------------------------------------
// A frame that leaps has no recorded costs yet when its view is new (the reference's benchmark renders every view once): this kernel
// predicts them.  Eight lanes per workgroup tile walk one ray each (the centres of the tile's eighths) through the 32^3 ESL bit volume in
// half-block strides and count the strides that lie in non-empty blocks: cost = the largest such count in samples + one per stride
// probed (what the ESL loop pays in empty space).  Early ray termination is not modelled (an upper estimate for opaque regions).
// Feeds tile_order_kernel like a recording does.  Placement only: the image does not depend on it.
__global__ __launch_bounds__(256)
void tile_estimate_kernel(const RayKernelArgs a, uint32_t tile_h, const uint32_t *__restrict__ esl_g, uint32_t *__restrict__ cost, uint32_t ntiles) {
	const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
	const uint32_t t = gid >> 3, probe = gid & 7u;                      // eight lanes per tile, one ray each
	uint32_t tile_x = 0, tile_y = 0;
	if (t < ntiles) tile_to_xy(a.tiles_x, a.tiles_y, t, t, tile_x, tile_y);
	const float edge = flmin(flmin(a.p.esl_block_size[0], a.p.esl_block_size[1]), a.p.esl_block_size[2]);
	uint32_t best = 0;
	do {
		if (t >= ntiles) break;
		// the centres of the tile's 4 x 2 eighths (one 8x8-pixel wave each in the 32x16 tile)
		const uint32_t px = (probe & 3u) * 8u + 4u, py = (probe >> 2) * (tile_h / 2u) + tile_h / 4u;
		const uint32_t lx = tile_x * 32u + px - a.phase_x, ly = tile_y * tile_h + py - a.phase_y;
		if (lx >= a.p.out_width || ly >= a.p.out_rows) continue;
		const PixelRay ray = pixel_ray(a, a.p.x0 + lx, frame_row(a, ly));
		if (!ray.alive) continue;
		const f3 origin = ray.origin, dir = ray.dir;
		const float kx = ray.kx, ky = ray.ky;
		const float longest = flmax(flmax(__builtin_fabsf(dir.x), __builtin_fabsf(dir.y)), __builtin_fabsf(dir.z));
		const float dk = 0.5f * edge / flmax(longest, 1e-6f);
		if (!(dk > 0.0f)) continue;
		const float strides_f = (ky - kx) / dk;
		const uint32_t strides = strides_f < 1.0f ? 1u : (strides_f > 400.0f ? 400u : (uint32_t) strides_f);
		uint32_t full = 0;
		for (uint32_t i = 0; i < strides; i++) {
			const float k = kx + ((float) i + 0.5f) * dk;
			const BlockIdx b = block_index(a, mk3(origin.x + dir.x * k, origin.y + dir.y * k, origin.z + dir.z * k));
			const uint32_t index = (b.z * VR_ESL_VOLUME_DIMS + b.y) & 0xffffu;
			if ((esl_g[index & (VR_ESL_VOLUME_SIZE - 1)] & (1u << (b.x & 31u))) == 0u) full++;
		}
		const float samples_per_stride = dk / flmax(a.p.ray_step, 1e-9f);
		const float est = (float) full * flmin(samples_per_stride, 4096.0f) + (float) strides;
		best = est > 4.0e9f ? 4000000000u : (uint32_t) est;
	} while (false);
	#pragma unroll
	for (uint32_t d = 1; d < 8u; d <<= 1) { const uint32_t o = __shfl_xor(best, d, 64); best = o > best ? o : best; }
	if (probe == 0u && t < ntiles) cost[t] = best;
}

hipError_t launch_tile_estimate(const RayKernelArgs &a, uint32_t tile_h, const uint32_t *esl, uint32_t *cost, uint32_t ntiles, hipStream_t stream) {
	hipLaunchKernelGGL(tile_estimate_kernel, dim3((ntiles * 8u + 255u) / 256u), dim3(256), 0, stream, a, tile_h, esl, cost, ntiles);
	return hipGetLastError();
}

hipError_t launch_tile_order(uint32_t *cost, uint32_t *order, uint32_t ntiles, hipStream_t stream) {
	hipLaunchKernelGGL(tile_order_kernel, dim3(1), dim3(kOrderThreads), 0, stream, cost, order, ntiles);
	return hipGetLastError();
}

// ---- choice between the two run copies per block of tiles (kLayoutRunDual) ------------------------------------------------------
// choice[t] = t, with kTileAltBit set where the frame recorded on the copy along y was cheaper than the frame recorded on the copy
// along z.  Decided per group of 64 consecutive tile numbers — one 8x8-tile block of the numbering, 256x128 pixels — from the SUMS of
// the tile costs, and for the copy along y only if it wins by 5 % (VR_DUAL_KEEP_PERCENT, tuning aid): single tile costs are noisy (they depend on what else ran on the
// CU), and tiles that read different copies share no cache lines — neighbours must agree (measured: alternating tiles +20 % frame
// time, a per-tile choice +12 % on the perspective oblique pose, where the two copies are nearly level).  Both costs NULL:
// alternating tiles (testing aid: the two copies meet at tile boundaries all over the frame).  Placement only.
__global__ __launch_bounds__(64)
void tile_choice_kernel(const uint32_t *__restrict__ cost_z, const uint32_t *__restrict__ cost_y, uint32_t *__restrict__ choice, uint32_t ntiles, uint32_t keep_percent) {
	const uint32_t t = blockIdx.x * 64u + threadIdx.x;
	bool alt;
	if (cost_z != nullptr && cost_y != nullptr) {
		uint64_t z = t < ntiles ? cost_z[t] : 0u, y = t < ntiles ? cost_y[t] : 0u;
		for (int d = 32; d >= 1; d >>= 1) { z += __shfl_xor(z, d, 64); y += __shfl_xor(y, d, 64); }
		alt = y * 100u < z * keep_percent;
	} else alt = ((t ^ (t >> 3)) & 1u) != 0u;
	if (t < ntiles) choice[t] = t | (alt ? kTileAltBit : 0u);
}

hipError_t launch_tile_choice(const uint32_t *cost_z, const uint32_t *cost_y, uint32_t *choice, uint32_t ntiles, hipStream_t stream) {
	static const uint32_t keep_percent = [] { const char *e = getenv("VR_DUAL_KEEP_PERCENT"); return e ? (uint32_t) atoi(e) : 95u; }();
	hipLaunchKernelGGL(tile_choice_kernel, dim3((ntiles + 63u) / 64u), dim3(64), 0, stream, cost_z, cost_y, choice, ntiles, keep_percent);
	return hipGetLastError();
}

}  // namespace vr
