// vr_slab.hip — pre-integrated (slab) classification for composite frames (include/vr_hip.h vr_hip_set_preintegration, DESIGN.md section
// 4.10): composite_slab and composite_slab_lit are the composite march (the family definition vr_composite_family.inc, declared here with
// SLAB set) whose samples take the mean of the transfer function between the previous sample's coordinate and their own — from the
// integral table K in LDS — in place of one lookup.
#include "vr_march.h"

namespace vr {

// The clipped composite's body with SLAB set: it always runs clip_segment (the host fills the identity clip when no clip is set, which
// changes no bit by contract), carries the reference's cue and tests the shadow per dense sample as a kernel argument, as composite_lit
// does, so slab frames with clip, with shadow and with both need no further family.  TRILINEAR and TRILINEAR_Q8 only; the rows of composite_lit.
#define VR_FAMILY_KERNEL composite_slab
#define VR_FAMILY_FLAGS  CLIP = true, SHADOW = false, LIT = false, SLAB = true, BACKDROP = false
#define VR_FAMILY_OUT    __restrict__
#include "vr_composite_family.inc"
// ... with the gradient lighting (vr_hip_set_lighting) in place of the cue
#define VR_FAMILY_KERNEL composite_slab_lit
#define VR_FAMILY_FLAGS  CLIP = true, SHADOW = false, LIT = true, SLAB = true, BACKDROP = false
#define VR_FAMILY_OUT    __restrict__
#include "vr_composite_family.inc"

// tf: the 128 entries and their running integral K behind them
hipError_t launch_composite_slab(const RayKernelArgs &args, const void *linear, const void *bricked, uint32_t bpv, const float *tf,
                                 const uint32_t *esl, void *out, TileSchedule sched, hipStream_t stream) {
	if (!args.slab_on) return hipErrorInvalidValue;
	return launch_composite_feature(args, linear, bricked, bpv, tf, esl, out, sched, stream, [&](auto row) {
		return !args.light_on ? VR_ROW_KERNEL(composite_slab, row) : VR_ROW_KERNEL(composite_slab_lit, row);
	});
}

}  // namespace vr
