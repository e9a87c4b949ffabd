// vr_raymarch.hip — the composite ray march: raymarch_kernel, raymarch_clipped (one body, vr_raymarch_body.inc) and their launcher.
#include "vr_march.h"

namespace vr {

// ---- the ray-march kernel ------------------------------------------------------------------------------------------

// raymarch_kernel and raymarch_clipped (a clipped frame, vr_hip_set_clip: the segment of every ray narrowed by clip_segment) are ONE body,
// vr_raymarch_body.inc, compiled twice with CLIP = false / true.  Two kernels, not a flag in the kernel argument: the hot variants sit at the
// 80-SGPR limit.  And the text itself inside each kernel, not a shared __device__ function template: as a function of its own the body is
// optimised before it is inlined, the loop vectoriser then decides the table-staging loops of the 64-bit-table and run-brick variants the
// other way, and those instantiations of the UNCLIPPED kernel take 17-28 more SGPRs (measured).
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void raymarch_kernel(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g,
                     const uint32_t *__restrict__ esl_g, uint32_t *__restrict__ out,
                     const uint32_t *__restrict__ tile_order, uint32_t *__restrict__ tile_cost) {
	constexpr bool CLIP = false, SHADOW = false, LIT = false, SLAB = false, BACKDROP = false;
#include "vr_raymarch_body.inc"
}
// ... of a clipped frame (vr_hip_set_clip): the linear array, the quad, voxel and oct bricks — never a run copy (launch_frame).  Its own
// name, so that the register tests of raymarch_kernel's instantiations count what they counted; tests/test_clip_model.py holds these
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void raymarch_clipped(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g,
                      const uint32_t *__restrict__ esl_g, uint32_t *__restrict__ out,
                      const uint32_t *__restrict__ tile_order, uint32_t *__restrict__ tile_cost) {
	static_assert(!is_run_layout(LAYOUT), "a clipped frame never reads a run copy");
	constexpr bool CLIP = true, SHADOW = false, LIT = false, SLAB = false, BACKDROP = false;
#include "vr_raymarch_body.inc"
}

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
	if (args.backdrop_on)                                        // a frame over an opaque layer (vr_hip_render_backdrop), whatever else is set: kernels of its own, in vr_backdrop.hip and vr_backdrop_slab.hip
		return args.slab_on ? launch_composite_backdrop_slab(args, linear, bricked, bpv, tf, esl, out, sched, stream)
		                    : launch_composite_backdrop(args, linear, bricked, bpv, tf, esl, out, sched, stream);
	if (args.slab_on)                                            // a pre-integrated frame (vr_hip_set_preintegration), clipped, shadowed, lit or not: kernels of its own, in vr_slab.hip
		return args.light_on ? launch_composite_slab_lit(args, linear, bricked, bpv, tf, esl, out, sched, stream)
		                     : launch_composite_slab(args, linear, bricked, bpv, tf, esl, out, sched, stream);
	if (args.light_on)                                           // a gradient-lit frame (vr_hip_set_lighting), shadowed or not: kernels of its own, in vr_light.hip
		return launch_composite_lit(args, linear, bricked, bpv, tf, esl, out, sched, stream);
	if (args.shadow_on)                                          // a shadowed frame (vr_hip_set_shadow): kernels of its own, in vr_shadow.hip
		return launch_raymarch_shadowed(args, linear, bricked, bpv, tf, esl, out, sched, stream);
	return select_variant(args, bricked != nullptr, bpv, [&](auto sampling, auto voxel, auto addr, auto layout, bool reads_linear) {
		constexpr int SAMPLING = decltype(sampling)::value, BPV = decltype(voxel)::value, ADDR = decltype(addr)::value, LAYOUT = decltype(layout)::value;
		constexpr uint32_t threads = variant_threads<ADDR, LAYOUT>();
		RayKernelArgs a = args;
		tile_grid(a.p.out_width, a.p.out_rows, a.phase_x, a.phase_y, threads, a.tiles_x, a.tiles_y);
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
		const uint32_t dynamic_lds = ((VR_PAD_LAYOUTS >> LAYOUT) & 1u) && !a.p.esl ? VR_RUN_LDS_PAD : 0;
		auto kernel = raymarch_kernel<SAMPLING, BPV, ADDR, LAYOUT>;
		if (a.clip_on) {                                         // a clipped frame: its own kernels, none of which reads a run copy (launch_frame asks for none)
			if constexpr (is_run_layout(LAYOUT)) return hipErrorInvalidValue;
			else kernel = raymarch_clipped<SAMPLING, BPV, ADDR, LAYOUT>;
		}
		hipLaunchKernelGGL(kernel, dim3(a.tiles_x * a.tiles_y), dim3(threads), dynamic_lds, stream,
		                   a, reads_linear ? linear : bricked, tf, esl, (uint32_t *) out, sched.order, sched.cost);
		return hipGetLastError();
	});
}

}  // namespace vr
