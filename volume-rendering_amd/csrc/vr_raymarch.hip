// vr_raymarch.hip — the composite ray march: raymarch_kernel, raymarch_clipped (one definition, vr_composite_family.inc, around one body,
// vr_raymarch_body.inc) and their launcher, which hands the feature frames to the units of their families.
#include "vr_march.h"

namespace vr {

// ---- the ray-march kernels ----------------------------------------------------------------------------------------------------------

// raymarch_kernel and raymarch_clipped (a clipped frame, vr_hip_set_clip: the segment of every ray narrowed by clip_segment) are ONE body,
// vr_raymarch_body.inc, in ONE kernel definition, vr_composite_family.inc (which says why a kernel per family and why the body is text),
// declared twice with CLIP = false / true.
#define VR_FAMILY_KERNEL raymarch_kernel
#define VR_FAMILY_FLAGS  CLIP = false, SHADOW = false, LIT = false, SLAB = false, BACKDROP = false
#define VR_FAMILY_OUT    __restrict__
#include "vr_composite_family.inc"
// ... of a clipped frame (vr_hip_set_clip): the linear array, the quad, voxel and oct bricks — never a run copy (launch_frame).  Its own
// name, so that the register tests of raymarch_kernel's instantiations count what they counted; tests/test_clip_model.py holds these
#define VR_FAMILY_KERNEL raymarch_clipped
#define VR_FAMILY_FLAGS  CLIP = true, SHADOW = false, LIT = false, SLAB = false, BACKDROP = false
#define VR_FAMILY_OUT    __restrict__
#include "vr_composite_family.inc"

// what launch_raymarch will do with these arguments (launch_frame asks before it launches)
RaymarchPlan plan_raymarch(const RayKernelArgs &a, bool have_bricked, uint32_t bpv) {
	if (have_bricked && (a.layout == kLayoutColumn || a.layout == kLayoutVoxCol)) {      // the column kernels: 512 threads = 32x16 pixels
		RaymarchPlan plan;
		plan.reads_linear = false;
		tile_grid(a.p.out_width, a.p.out_rows, a.phase_x, a.phase_y, 512u, plan.tiles_x, plan.tiles_y);
		return plan;
	}
	return select_variant(a, have_bricked, bpv, [&](auto, auto, auto addr, auto layout, bool reads_linear) {
		constexpr uint32_t threads = variant_threads<decltype(addr)::value, decltype(layout)::value>();
		RaymarchPlan plan;
		plan.reads_linear = reads_linear;
		tile_grid(a.p.out_width, a.p.out_rows, a.phase_x, a.phase_y, threads, plan.tiles_x, plan.tiles_y);
		plan.tile_h = threads / 32u;
		return plan;
	});
}

hipError_t launch_raymarch(const RayKernelArgs &args, const void *linear, const void *bricked, uint32_t bpv, const float *tf,
                           const uint32_t *esl, void *out, TileSchedule sched, hipStream_t stream) {
	if (bricked != nullptr && (args.layout == kLayoutColumn || args.layout == kLayoutVoxCol))      // orthogonal view along args.col_axis, full march, 1-byte voxels (launch_frame)
		return launch_colmarch(args, bricked, tf, out, stream);
	// The feature frames have kernels of their own, each family in a unit of its own with one launcher.  A frame over an opaque layer
	// (vr_hip_render_backdrop) first, whatever else is set: vr_backdrop_slab.hip with pre-integration, vr_backdrop.hip without; then a
	// pre-integrated frame (vr_hip_set_preintegration), clipped, shadowed, lit or not: vr_slab.hip; then a gradient-lit frame
	// (vr_hip_set_lighting), shadowed or not: vr_light.hip; then a shadowed frame (vr_hip_set_shadow): vr_shadow.hip.
	CompositeLauncher *const feature = args.backdrop_on ? (args.slab_on ? launch_composite_backdrop_slab : launch_composite_backdrop)
	                                 : args.slab_on     ? launch_composite_slab
	                                 : args.light_on    ? launch_composite_lit
	                                 : args.shadow_on   ? launch_raymarch_shadowed : nullptr;
	if (feature != nullptr) return feature(args, linear, bricked, bpv, tf, esl, out, sched, stream);
	// Run-brick frames are launched with 16 KiB of unused dynamic LDS: 3 instead of 4 workgroups per CU (24 waves).  Their waves
	// touch ~10 cache lines per step, 32 of them overflow the 256 lines of the 32 KiB L1 between two steps and the L2 catches only a
	// quarter of that reuse (measured: fabric requests -11 %, frame time -2 ... -5 % on those views; the VALU-bound quad-brick views
	// need all 32 waves and lose 10 % with the same padding).  Not with empty-space leaping: those rays are short, the frame time is
	// the tail of the few waves that probe a whole row of blocks, and fewer resident workgroups lengthen it (view 3: 1.53 -> 2.16 ms).
	// VR_RUN_LDS_PAD=0 builds without it (A/B).
#ifndef VR_RUN_LDS_PAD
#define VR_RUN_LDS_PAD 16384
#endif
#ifndef VR_PAD_LAYOUTS
#define VR_PAD_LAYOUTS ((1u << kLayoutRun) | (1u << kLayoutRunY) | (1u << kLayoutRunDual))
#endif
	const auto run_pad = [](auto row, const RayKernelArgs &a) -> uint32_t { return ((VR_PAD_LAYOUTS >> decltype(row)::layout) & 1u) && !a.p.esl ? VR_RUN_LDS_PAD : 0; };
	if (!args.clip_on)
		return launch_tiles<rows_all>(args, linear, bricked, bpv, stream, run_pad, [](auto row) { return VR_ROW_KERNEL(raymarch_kernel, row); },
		                              tf, esl, (uint32_t *) out, sched.order, sched.cost);
	// a clipped frame: its own kernels, none of which reads a run copy (launch_frame asks for none)
	return launch_tiles<rows_no_run>(args, linear, bricked, bpv, stream, run_pad, [](auto row) { return VR_ROW_KERNEL(raymarch_clipped, row); },
	                                 tf, esl, (uint32_t *) out, sched.order, sched.cost);
}

}  // namespace vr
