// vr_backdrop_slab.hip — pre-integrated composite frames over an opaque layer (include/vr_hip.h vr_hip_render_backdrop with
// vr_hip_set_preintegration): composite_backdrop_slab and composite_backdrop_slab_lit are composite_slab and
// composite_slab_lit (vr_slab.hip) with the BACKDROP flag set too (the family definition vr_composite_family.inc, declared here) — the rays
// stop at the layer's depth, the accumulated colour is blended over the layer's.  The point-classified families are vr_backdrop.hip.
#include "vr_march.h"

namespace vr {

// `out` carries no __restrict__ (vr_composite_family.inc says why)
#define VR_FAMILY_KERNEL composite_backdrop_slab
#define VR_FAMILY_FLAGS  CLIP = true, SHADOW = false, LIT = false, SLAB = true, BACKDROP = true
#define VR_FAMILY_OUT
#include "vr_composite_family.inc"
// ... with the gradient lighting (vr_hip_set_lighting) in place of the cue
#define VR_FAMILY_KERNEL composite_backdrop_slab_lit
#define VR_FAMILY_FLAGS  CLIP = true, SHADOW = false, LIT = true, SLAB = true, BACKDROP = true
#define VR_FAMILY_OUT
#include "vr_composite_family.inc"

// tf: the 128 entries and their running integral K behind them, as for launch_composite_slab
hipError_t launch_composite_backdrop_slab(const RayKernelArgs &args, const void *linear, const void *bricked, uint32_t bpv, const float *tf,
                                          const uint32_t *esl, void *out, TileSchedule sched, hipStream_t stream) {
	if (!args.backdrop_on || !args.slab_on) return hipErrorInvalidValue;
	return launch_composite_feature(args, linear, bricked, bpv, tf, esl, out, sched, stream, [&](auto row) {
		return !args.light_on ? VR_ROW_KERNEL(composite_backdrop_slab, row) : VR_ROW_KERNEL(composite_backdrop_slab_lit, row);
	});
}

}  // namespace vr
