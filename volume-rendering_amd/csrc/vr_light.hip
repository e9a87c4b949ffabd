// vr_light.hip — gradient lighting for composite frames (include/vr_hip.h vr_hip_set_lighting): composite_lit is the
// composite march (vr_raymarch_body.inc once more) whose dense samples take a Blinn-Phong term from the gradient of the interpolated field
// (vr_march.h light_sample) in place of the reference's cue, and the factor of a shadow behind it when one is set.
#include "vr_march.h"

namespace vr {

// The clipped composite's body with LIT set: it always runs clip_segment (the host fills the identity clip when no clip is set, which
// changes no bit by contract) and tests the shadow per dense sample as a kernel argument, so lighting with clip, with shadow and with both
// needs no further family.  TRILINEAR and TRILINEAR_Q8 only; the rows of raymarch_shadowed.
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void composite_lit(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g,
                   const uint32_t *__restrict__ esl_g, uint32_t *__restrict__ out,
                   const uint32_t *__restrict__ tile_order, uint32_t *__restrict__ tile_cost) {
	static_assert(!is_run_layout(LAYOUT) && SAMPLING != VR_SAMPLE_NEAREST, "a gradient-lit frame is TRILINEAR and never reads a run copy");
	constexpr bool CLIP = true, SHADOW = false, LIT = true, SLAB = false, BACKDROP = false;
#include "vr_raymarch_body.inc"
}

hipError_t launch_composite_lit(const RayKernelArgs &args, const void *linear, const void *bricked, uint32_t bpv, const float *tf,
                                const uint32_t *esl, void *out, TileSchedule sched, hipStream_t stream) {
	if (!args.light_on || (args.shadow_on && args.shadow_q == 0ull) || args.p.sampling == VR_SAMPLE_NEAREST) return hipErrorInvalidValue;
	return select_variant(args, bricked != nullptr, bpv, [&](auto sampling, auto voxel, auto addr, auto layout, bool reads_linear) {
		constexpr int SAMPLING = decltype(sampling)::value, BPV = decltype(voxel)::value, ADDR = decltype(addr)::value, LAYOUT = decltype(layout)::value;
		if constexpr (SAMPLING == VR_SAMPLE_NEAREST || is_run_layout(LAYOUT) || LAYOUT == kLayoutVoxel) return hipErrorInvalidValue;
		else {
			constexpr uint32_t threads = variant_threads<ADDR, LAYOUT>();
			RayKernelArgs a = args;
			tile_grid(a.p.out_width, a.p.out_rows, a.phase_x, a.phase_y, threads, a.tiles_x, a.tiles_y);
			hipLaunchKernelGGL((composite_lit<SAMPLING, BPV, ADDR, LAYOUT>), dim3(a.tiles_x * a.tiles_y), dim3(threads), 0, stream,
			                   a, reads_linear ? linear : bricked, tf, esl, (uint32_t *) out, sched.order, sched.cost);
			return hipGetLastError();
		}
	});
}

}  // namespace vr
