// vr_backdrop_slab.hip — pre-integrated composite frames over an opaque layer (include/vr_hip.h vr_hip_render_backdrop with
// vr_hip_set_preintegration): composite_backdrop_slab and composite_backdrop_slab_lit are composite_slab and
// composite_slab_lit (vr_slab.hip) with the BACKDROP flag of vr_raymarch_body.inc set — the rays stop at the layer's depth, the accumulated
// colour is blended over the layer's.  The point-classified families are vr_backdrop.hip.
#include "vr_march.h"

namespace vr {

// `out` carries no __restrict__: it may be the colour layer, which the body reads through an address (vr_march.h)
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void composite_backdrop_slab(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g,
                             const uint32_t *__restrict__ esl_g, uint32_t *out,
                             const uint32_t *__restrict__ tile_order, uint32_t *__restrict__ tile_cost) {
	static_assert(!is_run_layout(LAYOUT) && SAMPLING != VR_SAMPLE_NEAREST, "a backdrop frame is TRILINEAR and never reads a run copy");
	constexpr bool CLIP = true, SHADOW = false, LIT = false, SLAB = true, BACKDROP = true;
#include "vr_raymarch_body.inc"
}
// ... with the gradient lighting (vr_hip_set_lighting) in place of the cue
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void composite_backdrop_slab_lit(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g,
                                 const uint32_t *__restrict__ esl_g, uint32_t *out,
                                 const uint32_t *__restrict__ tile_order, uint32_t *__restrict__ tile_cost) {
	static_assert(!is_run_layout(LAYOUT) && SAMPLING != VR_SAMPLE_NEAREST, "a backdrop frame is TRILINEAR and never reads a run copy");
	constexpr bool CLIP = true, SHADOW = false, LIT = true, SLAB = true, BACKDROP = true;
#include "vr_raymarch_body.inc"
}

// tf: the 128 entries and their running integral K behind them, as for launch_composite_slab
hipError_t launch_composite_backdrop_slab(const RayKernelArgs &args, const void *linear, const void *bricked, uint32_t bpv, const float *tf,
                                          const uint32_t *esl, void *out, TileSchedule sched, hipStream_t stream) {
	if (!args.backdrop_on || !args.slab_on || args.backdrop_rgba == 0ull || args.backdrop_depth == 0ull || (args.shadow_on && args.shadow_q == 0ull) ||
	    args.p.sampling == VR_SAMPLE_NEAREST)
		return hipErrorInvalidValue;
	return select_variant(args, bricked != nullptr, bpv, [&](auto sampling, auto voxel, auto addr, auto layout, bool reads_linear) {
		constexpr int SAMPLING = decltype(sampling)::value, BPV = decltype(voxel)::value, ADDR = decltype(addr)::value, LAYOUT = decltype(layout)::value;
		if constexpr (SAMPLING == VR_SAMPLE_NEAREST || is_run_layout(LAYOUT) || LAYOUT == kLayoutVoxel) return hipErrorInvalidValue;
		else {
			constexpr uint32_t threads = variant_threads<ADDR, LAYOUT>();
			RayKernelArgs a = args;
			tile_grid(a.p.out_width, a.p.out_rows, a.phase_x, a.phase_y, threads, a.tiles_x, a.tiles_y);
			auto kernel = composite_backdrop_slab<SAMPLING, BPV, ADDR, LAYOUT>;
			if (a.light_on) kernel = composite_backdrop_slab_lit<SAMPLING, BPV, ADDR, LAYOUT>;
			hipLaunchKernelGGL(kernel, dim3(a.tiles_x * a.tiles_y), dim3(threads), 0, stream,
			                   a, reads_linear ? linear : bricked, tf, esl, (uint32_t *) out, sched.order, sched.cost);
			return hipGetLastError();
		}
	});
}

}  // namespace vr
