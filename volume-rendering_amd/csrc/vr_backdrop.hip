// vr_backdrop.hip — composite frames over an opaque layer (include/vr_hip.h vr_hip_render_backdrop / vr_hip_render_hybrid, DESIGN.md section
// 4.11): composite_backdrop and composite_backdrop_lit are the composite march (the family definition vr_composite_family.inc, declared
// here with BACKDROP set) whose rays stop at the depth of an RGBA8 layer and whose accumulated colour is blended over the layer's.  The
// pre-integrated families are vr_backdrop_slab.hip: two units, so that each compiles beside vr_raymarch.hip in the parallel make.
#include "vr_march.h"

namespace vr {

// The clipped composite's body with BACKDROP set: it always runs clip_segment (the host fills the identity clip when no clip is set, which
// changes no bit by contract), carries the reference's cue and tests the shadow per dense sample as a kernel argument, as composite_lit and
// composite_slab do, so backdrop frames with clip, with shadow and with both need no further family.  TRILINEAR and TRILINEAR_Q8 only; the
// rows of composite_lit.  `out` carries no __restrict__ (vr_composite_family.inc says why).
#define VR_FAMILY_KERNEL composite_backdrop
#define VR_FAMILY_FLAGS  CLIP = true, SHADOW = false, LIT = false, SLAB = false, BACKDROP = true
#define VR_FAMILY_OUT
#include "vr_composite_family.inc"
// ... with the gradient lighting (vr_hip_set_lighting) in place of the cue
#define VR_FAMILY_KERNEL composite_backdrop_lit
#define VR_FAMILY_FLAGS  CLIP = true, SHADOW = false, LIT = true, SLAB = false, BACKDROP = true
#define VR_FAMILY_OUT
#include "vr_composite_family.inc"

hipError_t launch_composite_backdrop(const RayKernelArgs &args, const void *linear, const void *bricked, uint32_t bpv, const float *tf,
                                     const uint32_t *esl, void *out, TileSchedule sched, hipStream_t stream) {
	if (!args.backdrop_on || args.slab_on) return hipErrorInvalidValue;
	return launch_composite_feature(args, linear, bricked, bpv, tf, esl, out, sched, stream, [&](auto row) {
		return !args.light_on ? VR_ROW_KERNEL(composite_backdrop, row) : VR_ROW_KERNEL(composite_backdrop_lit, row);
	});
}

}  // namespace vr
