// vr_backdrop.hip — composite frames over an opaque layer (include/vr_hip.h vr_hip_render_backdrop / vr_hip_render_hybrid, DESIGN.md section
// 4.11): composite_backdrop and composite_backdrop_lit are the composite march (vr_raymarch_body.inc once more) whose rays stop at the depth
// of an RGBA8 layer and whose accumulated colour is blended over the layer's.  The pre-integrated families are vr_backdrop_slab.hip: two
// units, so that each compiles beside vr_raymarch.hip in the parallel make.
#include "vr_march.h"

namespace vr {

// The clipped composite's body with BACKDROP set: it always runs clip_segment (the host fills the identity clip when no clip is set, which
// changes no bit by contract), carries the reference's cue and tests the shadow per dense sample as a kernel argument, as composite_lit and
// composite_slab do, so backdrop frames with clip, with shadow and with both need no further family.  TRILINEAR and TRILINEAR_Q8 only; the
// rows of composite_lit.  `out` carries no __restrict__: it may be the colour layer, which the body reads through an address (vr_march.h).
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void composite_backdrop(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g,
                        const uint32_t *__restrict__ esl_g, uint32_t *out,
                        const uint32_t *__restrict__ tile_order, uint32_t *__restrict__ tile_cost) {
	static_assert(!is_run_layout(LAYOUT) && SAMPLING != VR_SAMPLE_NEAREST, "a backdrop frame is TRILINEAR and never reads a run copy");
	constexpr bool CLIP = true, SHADOW = false, LIT = false, SLAB = false, BACKDROP = true;
#include "vr_raymarch_body.inc"
}
// ... with the gradient lighting (vr_hip_set_lighting) in place of the cue
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void composite_backdrop_lit(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g,
                            const uint32_t *__restrict__ esl_g, uint32_t *out,
                            const uint32_t *__restrict__ tile_order, uint32_t *__restrict__ tile_cost) {
	static_assert(!is_run_layout(LAYOUT) && SAMPLING != VR_SAMPLE_NEAREST, "a backdrop frame is TRILINEAR and never reads a run copy");
	constexpr bool CLIP = true, SHADOW = false, LIT = true, SLAB = false, BACKDROP = true;
#include "vr_raymarch_body.inc"
}

hipError_t launch_composite_backdrop(const RayKernelArgs &args, const void *linear, const void *bricked, uint32_t bpv, const float *tf,
                                     const uint32_t *esl, void *out, TileSchedule sched, hipStream_t stream) {
	if (!args.backdrop_on || args.slab_on || args.backdrop_rgba == 0ull || args.backdrop_depth == 0ull || (args.shadow_on && args.shadow_q == 0ull) ||
	    args.p.sampling == VR_SAMPLE_NEAREST)
		return hipErrorInvalidValue;
	return select_variant(args, bricked != nullptr, bpv, [&](auto sampling, auto voxel, auto addr, auto layout, bool reads_linear) {
		constexpr int SAMPLING = decltype(sampling)::value, BPV = decltype(voxel)::value, ADDR = decltype(addr)::value, LAYOUT = decltype(layout)::value;
		if constexpr (SAMPLING == VR_SAMPLE_NEAREST || is_run_layout(LAYOUT) || LAYOUT == kLayoutVoxel) return hipErrorInvalidValue;
		else {
			constexpr uint32_t threads = variant_threads<ADDR, LAYOUT>();
			RayKernelArgs a = args;
			tile_grid(a.p.out_width, a.p.out_rows, a.phase_x, a.phase_y, threads, a.tiles_x, a.tiles_y);
			auto kernel = composite_backdrop<SAMPLING, BPV, ADDR, LAYOUT>;
			if (a.light_on) kernel = composite_backdrop_lit<SAMPLING, BPV, ADDR, LAYOUT>;
			hipLaunchKernelGGL(kernel, dim3(a.tiles_x * a.tiles_y), dim3(threads), 0, stream,
			                   a, reads_linear ? linear : bricked, tf, esl, (uint32_t *) out, sched.order, sched.cost);
			return hipGetLastError();
		}
	});
}

}  // namespace vr
