// vr_light.hip — gradient lighting for composite frames (include/vr_hip.h vr_hip_set_lighting): composite_lit is the
// composite march (the family definition vr_composite_family.inc, declared here with LIT set) whose dense samples take a Blinn-Phong term
// from the gradient of the interpolated field (vr_march.h light_sample) in place of the reference's cue, and the factor of a shadow behind
// it when one is set.
#include "vr_march.h"

namespace vr {

// The clipped composite's body with LIT set: it always runs clip_segment (the host fills the identity clip when no clip is set, which
// changes no bit by contract) and tests the shadow per dense sample as a kernel argument, so lighting with clip, with shadow and with both
// needs no further family.  TRILINEAR and TRILINEAR_Q8 only; the rows of raymarch_shadowed.
#define VR_FAMILY_KERNEL composite_lit
#define VR_FAMILY_FLAGS  CLIP = true, SHADOW = false, LIT = true, SLAB = false, BACKDROP = false
#define VR_FAMILY_OUT    __restrict__
#include "vr_composite_family.inc"

hipError_t launch_composite_lit(const RayKernelArgs &args, const void *linear, const void *bricked, uint32_t bpv, const float *tf,
                                const uint32_t *esl, void *out, TileSchedule sched, hipStream_t stream) {
	if (!args.light_on) return hipErrorInvalidValue;
	return launch_composite_feature(args, linear, bricked, bpv, tf, esl, out, sched, stream, [](auto row) { return VR_ROW_KERNEL(composite_lit, row); });
}

}  // namespace vr
