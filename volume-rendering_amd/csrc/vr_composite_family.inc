// vr_composite_family.inc — the ONE definition of a composite-march kernel: every family of them (raymarch_kernel, raymarch_clipped,
// raymarch_shadowed, composite_lit, composite_slab*, composite_backdrop*) is this text, included once per family by the unit that holds it
// (DESIGN.md section 4.6).  In front of the include the unit defines
//   VR_FAMILY_KERNEL   the kernel's name (the register tests match on it);
//   VR_FAMILY_FLAGS    the initialisers of the body's five switches, in full: CLIP = .., SHADOW = .., LIT = .., SLAB = .., BACKDROP = ..
//   VR_FAMILY_OUT      the qualifier of `out`: __restrict__, or nothing for a BACKDROP family — its `out` may be the colour layer, which
//                      the body reads through an address (vr_march.h), so the two may alias;
// all three are undefined again at the end.
// A family is a kernel of its own, not a flag in the kernel argument: the hot variants sit at the 80-SGPR limit.  And the body is text
// inside each kernel, not a shared __device__ function template: as a function of its own it is optimised before it is inlined, the loop
// vectoriser then decides the table-staging loops of the 64-bit-table and run-brick variants the other way, and those instantiations of the
// UNCLIPPED kernel take 17-28 more SGPRs (measured; DESIGN.md section 4.6).
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void VR_FAMILY_KERNEL(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g,
                      const uint32_t *__restrict__ esl_g, uint32_t *VR_FAMILY_OUT out,
                      const uint32_t *__restrict__ tile_order, uint32_t *__restrict__ tile_cost) {
	constexpr bool VR_FAMILY_FLAGS;
	static_assert(!CLIP || !is_run_layout(LAYOUT), "a clipped frame never reads a run copy");
	static_assert(!(SHADOW || LIT || SLAB || BACKDROP) || (CLIP && SAMPLING != VR_SAMPLE_NEAREST),
	              "a shadowed, lit, slab or backdrop frame runs clip_segment and is TRILINEAR");
#include "vr_raymarch_body.inc"
}
#undef VR_FAMILY_KERNEL
#undef VR_FAMILY_FLAGS
#undef VR_FAMILY_OUT
