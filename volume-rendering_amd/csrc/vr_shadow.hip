// vr_shadow.hip — light-source shadows for composite frames (include/vr_hip.h vr_hip_set_shadow): shadow_build_kernel
// marches from every node of the light grid to the light and stores the transmittance as a byte; raymarch_shadowed is the composite march
// (the family definition vr_composite_family.inc, declared here with SHADOW set) whose dense samples are scaled by the trilinear
// interpolation of those bytes.
#include "vr_march.h"

namespace vr {

// ---- the builder: one lane per node, neighbouring lanes = neighbouring nodes along x (their light rays stay near-parallel) ----------------
// Steps 1-5 of the contract, the arithmetic of a composited TRILINEAR sample: texel coordinates fma(t, A, B), tri_issue / tri_resolve on the
// copy a TRILINEAR MIP frame along z reads, the linearly filtered transfer function from LDS.  Every fetch clamps its coordinates, so all
// lanes — finished ones, nodes without a segment, the lanes behind the last node — fetch in bounds and the loop has no per-lane control flow
// but the update of T; the wave leaves when none of its lanes marches any more (below the cutoff or past t_end).
template <int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void shadow_build_kernel(const RayKernelArgs a, const ShadowBuildArgs s, const void *__restrict__ vol, const float *__restrict__ tf_g,
                         uint8_t *__restrict__ q_out) {
	typedef LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)> L;
	constexpr uint32_t kThreads = L::threads;
	__shared__ float tf_w[VR_TF_SIZE + 1], dtf_w[VR_TF_SIZE + 1];      // alpha of the premultiplied TF and its deltas; entry 128 duplicates 127
	__shared__ __attribute__((aligned(16))) uint32_t lut[L::words];
	{
		const uint32_t t = threadIdx.x;
		if constexpr (L::max_dim != 0) stage_brick_tables<BPV, ADDR, LAYOUT>(a, lut);
		if (t <= VR_TF_SIZE) {
			const uint32_t i0 = t < VR_TF_SIZE ? t : VR_TF_SIZE - 1, i1 = t + 1 < VR_TF_SIZE ? t + 1 : VR_TF_SIZE - 1;
			const float w0 = tf_g[4 * i0 + 3], w1 = tf_g[4 * i1 + 3];
			tf_w[t] = w0; dtf_w[t] = w1 - w0;
		}
	}
	__syncthreads();

	const uint32_t S = s.dims, total = S * S * S;
	const uint32_t idx = blockIdx.x * kThreads + threadIdx.x;
	const bool node = idx < total;
	const uint32_t at = node ? idx : 0u;
	const uint32_t iz = at / (S * S), rem = at - iz * (S * S), iy = rem / S, ix = rem - iy * S;
	const f3 n = mk3(VR_FMA((float) ix, s.node_scale, -1.0f), VR_FMA((float) iy, s.node_scale, -1.0f), VR_FMA((float) iz, s.node_scale, -1.0f));
	const f3 d = mk3(s.light[0] - n.x, s.light[1] - n.y, s.light[2] - n.z);
	const float len2 = VR_FMA(d.z, d.z, VR_FMA(d.y, d.y, d.x * d.x));
	bool march = node && len2 > 0.0f;
	const float il = rsqrt_nr(march ? len2 : 1.0f);
	const f3 u = mk3(d.x * il, d.y * il, d.z * il);
	const float dist = len2 * il;
	float kx = 0.0f, ky = 0.0f;
	march = intersect(n, u, kx, ky) && march;
	if (s.clip_on) march = clip_segment(n, u, kx, ky) && march;
	float t_end = flmin(ky, dist);
	const float step = s.step, cutoff = s.cutoff;
	float t = flmax(kx, 0.0f) + step;
	f3 A = mk3(u.x * a.half_x, u.y * a.half_y, u.z * a.half_z);
	f3 B = mk3(VR_FMA(n.x, a.half_x, a.off_x), VR_FMA(n.y, a.half_y, a.off_y), VR_FMA(n.z, a.half_z, a.off_z));
	if (!march) { A = mk3(0.0f, 0.0f, 0.0f); B = A; t = 0.0f; t_end = -1.0f; }
	float T = 1.0f;
	bool active = march;
	const bool q8 = s.q8 != 0u;
	for (uint32_t steps = 0; steps < s.max_steps; steps++) {
		active = active && t <= t_end;
		if (__builtin_amdgcn_ballot_w64(active) == 0ull) break;
		const float xb = VR_FMA(t, A.x, B.x), yb = VR_FMA(t, A.y, B.y), zb = VR_FMA(t, A.z, B.z);
		const TriFetch<BPV, LAYOUT> f = tri_issue<BPV, ADDR, LAYOUT>(vol, a, lut, xb, yb, zb, true);
		const float raw = q8 ? tri_resolve<BPV, LAYOUT, true>(f, a, xb, yb, zb) : tri_resolve<BPV, LAYOUT, false>(f, a, xb, yb, zb);
		const float tb = __builtin_amdgcn_fmed3f(VR_FMA(raw, a.tf_scale, -0.5f), 0.0f, (float) (VR_TF_SIZE - 1));
		const uint32_t i = (uint32_t) (int) tb;
		const float fr = __builtin_amdgcn_fractf(tb), w = q8 ? filter_weight<true>(fr) : fr;
		const float alpha = VR_FMA(w, dtf_w[i], tf_w[i]);
		if (active) {
			T = T * (1.0f - alpha);
			if (T < cutoff) { T = 0.0f; active = false; }
		}
		t += step;
	}
	if (node) {
		const float scaled = T * 255.0f;
		q_out[idx] = (uint8_t) (scaled + 0.5f);
	}
}

hipError_t launch_shadow_build(const RayKernelArgs &args, const ShadowBuildArgs &s, const void *linear, const void *bricked, uint32_t bpv,
                               const float *tf, uint8_t *q_out, hipStream_t stream) {
	if (args.p.sampling != VR_SAMPLE_TRILINEAR || s.dims < 2u || s.dims > 256u) return hipErrorInvalidValue;
	return select_variant(args, bricked != nullptr, bpv, [&](auto sampling, auto voxel, auto addr, auto layout, bool reads_linear) {
		constexpr int SAMPLING = decltype(sampling)::value, BPV = decltype(voxel)::value, ADDR = decltype(addr)::value, LAYOUT = decltype(layout)::value;
		if constexpr (SAMPLING != VR_SAMPLE_TRILINEAR || is_run_layout(LAYOUT) || LAYOUT == kLayoutVoxel) return hipErrorInvalidValue;
		else {
			constexpr uint32_t threads = variant_threads<ADDR, LAYOUT>();
			const uint32_t total = s.dims * s.dims * s.dims;
			hipLaunchKernelGGL((shadow_build_kernel<BPV, ADDR, LAYOUT>), dim3((total + threads - 1u) / threads), dim3(threads), 0, stream,
			                   args, s, reads_linear ? linear : bricked, tf, q_out);
			return hipGetLastError();
		}
	});
}

// ---- the shadowed composite frame ---------------------------------------------------------------------------------------------------------
// raymarch_clipped with SHADOW set: it always runs clip_segment (the host fills the identity clip when no clip is set, which changes no bit
// by contract), so shadow with clip needs no fourth family.  TRILINEAR and TRILINEAR_Q8 only; the clipped table without its NEAREST rows.
#define VR_FAMILY_KERNEL raymarch_shadowed
#define VR_FAMILY_FLAGS  CLIP = true, SHADOW = true, LIT = false, SLAB = false, BACKDROP = false
#define VR_FAMILY_OUT    __restrict__
#include "vr_composite_family.inc"

hipError_t launch_raymarch_shadowed(const RayKernelArgs &args, const void *linear, const void *bricked, uint32_t bpv, const float *tf,
                                    const uint32_t *esl, void *out, TileSchedule sched, hipStream_t stream) {
	if (!args.shadow_on) return hipErrorInvalidValue;
	return launch_composite_feature(args, linear, bricked, bpv, tf, esl, out, sched, stream, [](auto row) { return VR_ROW_KERNEL(raymarch_shadowed, row); });
}

}  // namespace vr
