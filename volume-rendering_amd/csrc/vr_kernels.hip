// vr_kernels.hip — the column marches (orthogonal views along a volume axis): colmarch_kernel, colmarch_nearest_kernel, voxcol_tri_kernel,
// voxcol_pairs_kernel, what they share, and their launcher.  The other kernel units: vr_raymarch.hip, vr_project.hip, vr_schedule.hip, vr_builders.hip.
#include "vr_march.h"
#include <type_traits>

namespace vr {

// ---- the column march (kLayoutColumn, round 4) -----------------------------------------------------------------------------------
//
// Orthogonal views along a volume axis m, full march (no leaping, no early termination).  What makes them special (measured on the
// benchmark poses, scripts: every 8x8-pixel tile of the three axis-aligned views): all rays of a wave share kx bit for bit, so they
// share the whole k sequence, and with the direction's lateral components at most rounding noise (4e-8) a ray stays in ONE cell column
// (u,v) but for at most one cell flip per lateral axis.  The march therefore runs on wave-uniform state:
//   * the cell along m of a sample is the same for all 64 lanes: k += step, fma, float -> int, v_readfirstlane — four vector
//     instructions per sample instead of the 15 + 3 LDS lookups of the general address chain;
//   * ONE aligned 16-byte gather per lane and WINDOW (four consecutive quad elements of the lane's column = three cells, vr_device.h),
//     prefetched kColDepth windows ahead with exact s_waitcnt vmcnt accounting (one gather per window: static);
//   * the transparency test is done ONCE per window on all four elements: a window that is transparent for every live lane lets its
//     ~3 samples pass with the uniform chain alone (exact: every pair of elements the samples would test is part of the window);
//   * a lane whose column flips (monotone coordinate: at most once per axis, at the smallest float t with cell(t) != cell(kx), found by
//     bisection once per ray) reads the column of the state PREDICTED for a window's first sample; a window whose samples may see a
//     different state (t inside the window's k range, or between prediction and truth) takes the careful path: explicit per-sample
//     fetches from each lane's true column.
// Waves whose live lanes do not share kx and the coordinate along m (none on pose (0,0,0) and (90,0,0), 256 of 65536 on (180,90,0)),
// whose columns would flip by more than one cell, or whose lateral spread leaves the 32-bit offset range, march per lane with explicit
// fetches from the same copy (exact; pipelined: col_lane_march).  Arithmetic per composited sample is the general kernel's, expression by expression.
//
// Three kernels march this way: colmarch_kernel (TRILINEAR, quad-element windows), colmarch_nearest_kernel (NEAREST, voxel windows)
// and voxcol_tri_kernel (TRILINEAR, voxel windows).  What they share is written once, below: the ray of a lane (col_ray_setup), the
// test for the column path (col_wave_eligibility), the 64-sample k batch (ColBatch), the flip events (col_bisect, col_sort_events,
// ColFrontier), the two inner loops of a window (col_skip_window, col_for_window_samples), the TRILINEAR sample (col_tri_sample) and
// the end (col_drain, col_store).  A kernel spells out only what is its own: how a window is gathered and unpacked, where a sample's
// voxels come from, and (NEAREST) the reference's unfused sample arithmetic.
#ifndef VR_COL_DEPTH
#define VR_COL_DEPTH 3
#endif
#ifndef VR_COL_WAVES
#define VR_COL_WAVES 4
#endif
constexpr int kColDepth = VR_COL_DEPTH, kColSlots = kColDepth + 1;

__device__ __forceinline__ void managed_load128_s(u32x4 &dst, uint32_t byte_offset, uint64_t base) {     // window gather: scalar base + per-lane offset
	asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(dst) : "v"(byte_offset), "s"(base));
}
template <int I> __device__ __forceinline__ float comp3(const f3 &v) { return I == 0 ? v.x : (I == 1 ? v.y : v.z); }

// the eight corner voxels of a sample out of the two quad elements along m (w0 = march index i, w1 = i + 1) -> trilinear value;
// element bytes are (u,v), (u+1,v), (u,v+1), (u+1,v+1) with (u,v) the lateral axes of m in increasing order; lerps in x, y, z order
template <int M, bool Q8>
__device__ __forceinline__ float col_resolve(uint32_t w0, uint32_t w1, float max_x, float max_y, float max_z, float xb, float yb, float zb) {
	const float ax = filter_weight<Q8>(__builtin_amdgcn_fractf(__builtin_amdgcn_fmed3f(xb, 0.0f, max_x)));
	const float ay = filter_weight<Q8>(__builtin_amdgcn_fractf(__builtin_amdgcn_fmed3f(yb, 0.0f, max_y)));
	const float az = filter_weight<Q8>(__builtin_amdgcn_fractf(__builtin_amdgcn_fmed3f(zb, 0.0f, max_z)));
	const float p0 = (float) (w0 & 0xffu), p1 = (float) ((w0 >> 8) & 0xffu), p2 = (float) ((w0 >> 16) & 0xffu), p3 = (float) (w0 >> 24);
	const float q0 = (float) (w1 & 0xffu), q1 = (float) ((w1 >> 8) & 0xffu), q2 = (float) ((w1 >> 16) & 0xffu), q3 = (float) (w1 >> 24);
	float v000, v100, v010, v110, v001, v101, v011, v111;
	if (M == 2)      { v000 = p0; v100 = p1; v010 = p2; v110 = p3; v001 = q0; v101 = q1; v011 = q2; v111 = q3; }      // (u,v) = (x,y), pair along z
	else if (M == 1) { v000 = p0; v100 = p1; v001 = p2; v101 = p3; v010 = q0; v110 = q1; v011 = q2; v111 = q3; }      // (u,v) = (x,z), pair along y
	else             { v000 = p0; v010 = p1; v001 = p2; v011 = p3; v100 = q0; v110 = q1; v101 = q2; v111 = q3; }      // (u,v) = (y,z), pair along x
	const float c00 = lerp(v000, v100, ax), c10 = lerp(v010, v110, ax);
	const float c01 = lerp(v001, v101, ax), c11 = lerp(v011, v111, ax);
	const float c0 = lerp(c00, c10, ay), c1 = lerp(c01, c11, ay);
	return lerp(c0, c1, az);
}

// ---- what the column kernels share ---------------------------------------------------------------------------------------------------

// The transparent march runs on a dozen scalars; everything else the DENSE path needs (clamp bounds, shading constants, the light,
// the view direction) is read again from the kernel-argument segment where it is used, through a pointer the compiler cannot see
// through — kept live across the march those ~25 scalars push a kernel past the 80 SGPRs that 8 waves per SIMD allow, and the
// compiler then spills scalars into VGPR lanes inside the window loop (RayKernelArgs is the first argument: offset 0).
typedef const RayKernelArgs __attribute__((address_space(4))) *ColConstArgs;
struct ColKernelArguments { RayKernelArgs a; const uint8_t *copy; const float *tf_g; uint32_t *out; };      // the kernels' parameter list (the same for all three) as it lies in that segment
typedef const ColKernelArguments __attribute__((address_space(4))) *ColConstKernelArguments;
__device__ __forceinline__ ColConstArgs col_dense_args() { ColConstArgs q = (ColConstArgs) __builtin_amdgcn_kernarg_segment_ptr(); asm volatile("" : "+s"(q)); return q; }
// the same value in every lane, formed by the vector unit: moved to a scalar register so that it does not occupy a VGPR for the whole march
__device__ __forceinline__ float uni(float v) { return __uint_as_float(rfl(__float_as_uint(v))); }
__device__ __forceinline__ uint32_t col_lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }      // 0 .. 63

// the transfer function and the difference to each entry's successor (a lookup is fma(weight, delta, entry)) into LDS; no barrier
__device__ __forceinline__ void stage_tf_with_deltas(f4 (&tf_l)[VR_TF_SIZE + 1], f4 (&dtf_l)[VR_TF_SIZE + 1], const float *__restrict__ tf_g) {
	const uint32_t t = threadIdx.x;
	if (t <= VR_TF_SIZE) {
		const f4 *tf4 = (const f4 *) tf_g;
		const uint32_t i0 = t < VR_TF_SIZE ? t : VR_TF_SIZE - 1, i1 = t + 1 < VR_TF_SIZE ? t + 1 : VR_TF_SIZE - 1;
		const f4 c0 = tf4[i0], c1 = tf4[i1];
		tf_l[t] = c0;
		f4 d; d.x = c1.x - c0.x; d.y = c1.y - c0.y; d.z = c1.z - c0.z; d.w = c1.w - c0.w;
		dtf_l[t] = d;
	}
}

// The ray of a lane.  Lanes outside the buffer or without a segment stay in the wave (the batched sample sequence lives in all 64
// lanes): `alive` is false, ky = -1 (also what the final store reads "no segment" from).
struct ColRay {
	bool in_frame, alive;
	uint32_t out_index;                 // where the pixel goes: 0xffffffff for lanes outside the buffer (frames are at most 65535 x 65535 pixels, validate_params: every real index is smaller)
	uint32_t org_slot;                  // byte offset of the thread's origin in org_l
	f3 dir, origin;
	float kx, ky, step;
	uint64_t alive_mask;                // 0: nothing to march — the kernel stores 0 for the lanes in the frame and returns
};
// (the march does not keep the ray origin in three registers: the samples that are shaded — the dense path is bound by its vector
// instructions — read it back from the thread's own LDS slot, one ds_read_b128)
__device__ __forceinline__ f3 col_origin_again(const f4 (&org_l)[512], uint32_t &org_slot) {
	pin(org_slot);
	const f4 o4 = *(const f4 *) ((const char *) org_l + org_slot);
	return mk3(o4.x, o4.y, o4.z);
}
__device__ __forceinline__ void col_ray_setup(const RayKernelArgs &a, f4 (&org_l)[512], ColRay &r) {
	uint32_t tile_x, tile_y;
	tile_to_xy<VR_COL_XCD_MODE>(a.tiles_x, a.tiles_y, blockIdx.x, blockIdx.x, tile_x, tile_y);
	uint32_t lx, ly;
	lane_pixel<512u, true>(a, tile_x, tile_y, lx, ly);
	r.in_frame = lx < a.p.out_width && ly < a.p.out_rows;
	r.out_index = r.in_frame ? ly * a.p.out_width + lx : 0xffffffffu;

	// (perspective is wave-uniform and never true here: the host never launches these kernels for a perspective view)
	const PixelRay ray = pixel_ray<true>(a, a.p.x0 + lx, frame_row(a, ly));
	r.dir = ray.dir; r.origin = ray.origin;
	r.org_slot = threadIdx.x * (uint32_t) sizeof(f4);
	{ f4 o4; o4.x = r.origin.x; o4.y = r.origin.y; o4.z = r.origin.z; o4.w = 0.0f; org_l[threadIdx.x] = o4; }      // read by this thread only: no barrier
	r.kx = ray.kx; r.ky = ray.ky;
	r.step = a.p.ray_step;
	const bool alive = r.in_frame && ray.alive;
	r.alive = alive;
	r.alive_mask = __builtin_amdgcn_ballot_w64(alive);
	if (!alive) r.ky = -1.0f;
}

// Can this wave take the column path?  All live lanes share kx and their coordinate along m (`cm`: one k sequence, one cell along m), a
// sample advances between 1/64 and 1 cell along m (a window is never skipped, and holds a bounded number of samples), and no lane's
// lateral cell (cell_u / cell_v of k; monotone in k, so the two ends of the segment tell) changes by more than one.
struct ColWave {
	int leader;                         // the first live lane
	float kx_l, cm_l;                   // its kx and coordinate along m: the wave's
	int cu0, cv0, cu1, cv1;             // lateral cells at the two ends of the segment (lanes without a segment ride along in the leader's column)
	uint64_t flips_u, flips_v;          // lanes whose column changes along u / v
	bool ok;
};
template <class CellU, class CellV>
__device__ __forceinline__ void col_wave_eligibility(const ColRay &r, float cm, float advance, CellU cell_u, CellV cell_v, ColWave &w) {
	w.leader = __builtin_ctzll(r.alive_mask);
	w.kx_l = rlane(r.kx, w.leader); w.cm_l = rlane(cm, w.leader);
	w.ok = __builtin_amdgcn_ballot_w64(r.alive && (__float_as_uint(r.kx) != __float_as_uint(w.kx_l) || __float_as_uint(cm) != __float_as_uint(w.cm_l))) == 0ull;
	w.ok = w.ok && __builtin_amdgcn_ballot_w64(!(advance >= (1.0f / 64.0f) && advance <= 1.0f)) == 0ull;
	w.cu0 = cell_u(r.kx); w.cv0 = cell_v(r.kx);
	w.cu1 = cell_u(r.ky); w.cv1 = cell_v(r.ky);
	{
		const int lu = __builtin_amdgcn_readlane(w.cu0, w.leader), lv = __builtin_amdgcn_readlane(w.cv0, w.leader);
		if (!r.alive) { w.cu0 = w.cu1 = lu; w.cv0 = w.cv1 = lv; }
	}
	w.flips_u = __builtin_amdgcn_ballot_w64(w.cu0 != w.cu1); w.flips_v = __builtin_amdgcn_ballot_w64(w.cv0 != w.cv1);
	w.ok = w.ok && __builtin_amdgcn_ballot_w64((w.cu1 - w.cu0) * (w.cu1 - w.cu0) > 1 || (w.cv1 - w.cv0) * (w.cv1 - w.cv0) > 1) == 0ull;
}
// One gather address for the wave: a scalar base and unsigned 32-bit VGPR offsets.  `ref` = the byte offset of the leader's column in the
// copy, `rel0` = this lane's column relative to it; false if a lane's column, or the step to the column it flips to, is 2^28 bytes or
// more away (the offsets are biased by 2^30).  stride_u / stride_v: bytes between lateral blocks.
__device__ __forceinline__ bool col_lane_offsets(const ColWave &w, uint64_t stride_u, uint64_t stride_v, int64_t &ref, int64_t &rel0) {
	ref = (int64_t) col_lateral_offset64((uint32_t) __builtin_amdgcn_readlane(w.cu0, w.leader), (uint32_t) __builtin_amdgcn_readlane(w.cv0, w.leader), stride_u, stride_v);
	rel0 = (int64_t) col_lateral_offset64((uint32_t) w.cu0, (uint32_t) w.cv0, stride_u, stride_v) - ref;
	const int64_t du64 = (int64_t) col_axis_offset64((uint32_t) w.cu1, stride_u, kColWindowBytes) - (int64_t) col_axis_offset64((uint32_t) w.cu0, stride_u, kColWindowBytes);
	const int64_t dv64 = (int64_t) col_axis_offset64((uint32_t) w.cv1, stride_v, kColRowBytes) - (int64_t) col_axis_offset64((uint32_t) w.cv0, stride_v, kColRowBytes);
	const int64_t lim = 1ll << 28;
	return __builtin_amdgcn_ballot_w64(rel0 <= -lim || rel0 >= lim || du64 <= -lim || du64 >= lim || dv64 <= -lim || dv64 >= lim) == 0ull;
}
__device__ __forceinline__ uint64_t col_scalar_base(const uint8_t *copy, int64_t ref) {      // copy + ref - 2^30, in scalar registers
	const uint64_t b = (uint64_t) (uintptr_t) copy + (uint64_t) ref - (1ull << 30);
	return ((uint64_t) rfl((uint32_t) (b >> 32)) << 32) | rfl((uint32_t) b);
}
// Explicit fetch from a QUAD-ELEMENT window copy (kCopyCol*, march axis M): the address of the element pair (march index i, i + 1) of a
// texel-space position — 8 adjacent bytes of one window, 4-byte aligned — given the copy's base, the clamp maxima, its lateral blocks
// along u and its windows per column.  Clamp addressing: any position is in bounds.  64-bit: the copy may exceed 4 GiB.
template <int M>
__device__ __forceinline__ const uint8_t *col_pair_address(const RayKernelArgs &a, const uint8_t *copy_p, float mx, float my, float mz, uint32_t blocks_u, uint32_t windows,
                                                           float xb, float yb, float zb) {
	constexpr int U = M == 0 ? 1 : 0, V = M == 2 ? 1 : 2;
	const int ix = (int) __builtin_amdgcn_fmed3f(xb, 0.0f, mx), iy = (int) __builtin_amdgcn_fmed3f(yb, 0.0f, my), iz = (int) __builtin_amdgcn_fmed3f(zb, 0.0f, mz);
	const uint32_t iu = (uint32_t) (U == 0 ? ix : iy), iv = (uint32_t) (V == 1 ? iy : iz), im = (uint32_t) (M == 0 ? ix : (M == 1 ? iy : iz));
	const uint32_t wq = __umulhi(im, 0xAAAAAAABu) >> 1, sub = im - wq * 3u;
	const uint32_t block = col_lateral_block(iu, iv, blocks_u) * windows + wq;
	const uint32_t in_block = col_in_block(iu, iv) + sub * 4u;      // < 256: summed in 32 bits
	const uint8_t *p = copy_p + ((uint64_t) block * kColBlockBytes + in_block);
	return VR_BC_POINTER(a, const uint8_t *, p, 8u);
}

// The wave-uniform sample sequence, 64 samples at a time: lane j of `kvec` holds k of sample n + j, `wvec` the window its cell along m
// lies in (cell_to_window: the kernel's own cell arithmetic and cells per window).  The reference forms k by repeated fp32 additions
// k += step.  Inside one binade [2^e, 2^(e+1)) every k is a multiple of u = 2^(e-23), and fl(k + step) = k + round_u(step) whatever k
// is — unless step's part below u is exactly u / 2 (a tie, broken by k's parity) — so the sequence is an EXACT arithmetic progression
// there: k_(n+j) = fma(j, delta, k_n) with delta = fl(k_n + step) - k_n, no rounding (every term is a multiple of u inside the binade).
// A batch that would cross a binade, a tie, or k <= 2^-102 is formed by the 64 sequential additions instead (lane j keeps the j-th
// sum): a handful of batches per ray.
struct ColBatch {
	float kvec, knext;                  // knext: k of the next batch's first sample (scalar)
	int wvec;
	template <class W> __device__ __forceinline__ void refill(float step, uint32_t lane_i, W cell_to_window) {
		const float kbase = knext;
		const float k1 = kbase + step, delta = k1 - kbase, low = step - delta;           // delta = round_u(step); low = what the rounding dropped (both exact)
		const uint32_t e = __float_as_uint(kbase) >> 23;                                  // kbase >= 0: the biased exponent
		const float half_ulp = __uint_as_float((e > 24u ? e - 24u : 1u) << 23);
		const float kend = VR_FMA(64.0f, delta, kbase);
		const bool fast = rfl((e > 24u && (__float_as_uint(kend) >> 23) == e && __builtin_fabsf(low) != half_ulp && delta > 0.0f) ? 1u : 0u) != 0u;
		if (fast) {
			kvec = VR_FMA((float) lane_i, delta, kbase);
			knext = uni(kend);
		} else {
			float kc = kbase;
			#pragma nounroll
			for (uint32_t j = 0; j < 64u; j++) { kvec = lane_i == j ? kc : kvec; kc = kc + step; }
			knext = uni(kc);
		}
		wvec = cell_to_window(kvec);                                                     // (may leave 0 .. nw-1 past the exit)
	}
};
// the window the march starts in (0 .. nw-1 for the first sample of a live ray)
__device__ __forceinline__ int col_first_window(const ColBatch &b, uint32_t nw) {
	const int cur = __builtin_amdgcn_readlane(b.wvec, 0);
	return cur < 0 ? 0 : (cur > (int) nw - 1 ? (int) nw - 1 : cur);
}
// Hang / bounds guard: a ray cannot need more windows than lie ahead of its first one in march direction; past the last of them
// every k exceeds every ky and `live` empties at the next rotation, i.e. at most 2 * slots windows later.  Those — and the
// windows prefetched beyond — are read without a clamp: neighbouring blocks' windows, or the kColPadBytes of zeroes at both
// ends of the copy (64 windows).
static_assert(2 * kColSlots + kColDepth + 4 <= 64, "kColPadBytes");
__device__ __forceinline__ int col_window_budget(int dsign, uint32_t nw, int cur, int slots) { return (dsign > 0 ? (int) nw - cur : cur + 1) + 2 * slots; }

// The two inner loops of a window step.  The samples of window `cur` are consecutive lanes of the batch, from `pos`; the window may go
// on in the next batch (`refill`: the kernel's binding of ColBatch::refill).  A window of C cells holds at most 64 C + 1 samples (a
// sample advances >= 1/64 cell), i.e. it ends within C + 2 batches: `bound` is a hang guard.
template <class Refill>
__device__ __forceinline__ void col_skip_window(const ColBatch &b, int &pos, int cur, int bound, Refill refill) {      // a transparent window: its samples just pass
	for (int batches = 0; batches < bound; batches++) {
		pos += __builtin_popcountll(__builtin_amdgcn_ballot_w64(b.wvec == cur));
		if (pos < 64) break;
		refill(); pos = 0;
	}
	pos = pos < 64 ? pos : 63;
}
template <class Refill, class Body>
__device__ __forceinline__ void col_for_window_samples(const ColBatch &b, int &pos, int cur, int bound, Refill refill, Body body) {      // body(k), or body(k, the sample's lane in the batch), for every sample of the window
	for (int batches = 0; batches < bound; batches++) {
		const int cnt = __builtin_popcountll(__builtin_amdgcn_ballot_w64(b.wvec == cur));
		for (int i = pos; i < pos + cnt; i++) {
			if constexpr (std::is_invocable_v<Body, float, int>) body(rlane(b.kvec, i), i);
			else body(rlane(b.kvec, i));
		}
		pos += cnt;
		if (pos < 64) break;
		refill(); pos = 0;
	}
	pos = pos < 64 ? pos : 63;
}

// The per-lane march of the waves that cannot take the column path (live lanes that do not share kx bit for bit — on pose (180,90,0)
// one row of waves, where origin.x leaves 2.0 by one ulp —, a rectangle above 64 columns, offsets out of range, forced column frames):
// every lane marches its own k with explicit fetches from its true column.  Exact as before, and software-pipelined: the fetch of sample
// n + DEPTH is issued before sample n is consumed, so a sample costs its instructions instead of one memory round trip (a fallback wave of
// the 1025-sample benchmark march took 0.4 ms at one round trip per sample and ended the frame 0.25-0.3 ms after every other wave).
//   * Two running values instead of a ring of k's: `k` (the sample consumed) and k_issue (the sample fetched) go through the same
//     sequential k += step from the same start, so every k keeps the bits the reference's loop gives it.
//   * issue(kk, slot) forms the address of the sample at kk as the unpipelined fetch did and starts ONE managed load (vr_march.h:
//     the compiler does not see it, or it would wait for everything at the loop's back edge) into the slot's own registers;
//     consume(slot) is the kernel's sample() on what landed there.  The loop is written once per slot, rotated: no register copies.
//     Loads the compiler issues inside consume (the shading fetch) only add to the counter: managed_wait<DEPTH> then waits for more.
//   * Fetches run DEPTH samples past a lane's ky, and from kx on for lanes without a segment (they did before, too: every lane of a wave
//     fetches for as long as one lane is live).  Any position is in bounds: col_pair_address clamps its three indices with v_med3 and
//     colmarch_nearest_kernel's voxel_address with map_float_int (float -> int saturates, NaN gives 0), and the bounds-checked build
//     holds both addresses against the copy (VR_BC_POINTER inside them) like every other managed load.
#ifndef VR_COL_LANE_DEPTH
#define VR_COL_LANE_DEPTH 6
#endif
constexpr int kColLaneDepth = VR_COL_LANE_DEPTH;
template <int DEPTH, class Slot, class Issue, class Consume>
__device__ __forceinline__ void col_lane_march(float &k, float step, const float &ky, uint64_t &live, Issue issue, Consume consume) {
	static_assert(DEPTH >= 1 && DEPTH <= 16, "one load per slot: vmcnt(DEPTH)");
	Slot slot[DEPTH + 1];
	slot[DEPTH] = 0;
	float k_issue = k;
	static_for<0, DEPTH>([&](auto j) { issue(k_issue, slot[j.value]); k_issue += step; });
	while (live != 0ull) {
		static_for<0, DEPTH + 1>([&](auto jc) {
			constexpr int c = decltype(jc)::value, n = (c + DEPTH) % (DEPTH + 1);
			if (live != 0ull) {
				issue(k_issue, slot[n]); k_issue += step;
				__builtin_amdgcn_sched_barrier(0);
				pin(slot[c]); managed_wait<DEPTH>(); pin(slot[c]);
				consume(slot[c]);
				k += step;
				live &= __builtin_amdgcn_fcmpf(k, ky, kFcmpOLE);
			}
		});
	}
	static_for<0, DEPTH + 1>([&](auto j) { pin(slot[j.value]); });      // nothing in flight into registers the kernel releases (col_drain)
	managed_wait<0>();
	static_for<0, DEPTH + 1>([&](auto j) { pin(slot[j.value]); });
}

// Column flips.  A lane's lateral cell changes at the smallest float t in (kx, ky] with cell(t) != cell(kx): bisection over the
// positive float bit patterns, once per ray; returns t's bits (kx's for a lane that does not flip).
template <class Cell>
__device__ __forceinline__ uint32_t col_bisect(const ColRay &r, bool flipping, int c0, Cell cell) {
	uint32_t lo = __float_as_uint(r.kx), hi = __float_as_uint(r.ky);
	if (!flipping) hi = lo;
	for (int it = 0; it < 34 && __builtin_amdgcn_ballot_w64(hi - lo > 1u) != 0ull; it++) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		const bool same = cell(__uint_as_float(mid)) == c0;
		if (hi - lo > 1u) { if (same) lo = mid; else hi = mid; }
	}
	return hi;
}
// Flip events (colmarch_kernel, colmarch_nearest_kernel).  What the march needs of t is only the WINDOW Wt the position k = t lies in:
// the coordinate along m and its cell are monotone in k, so every sample in a window before Wt (in march order) has k < t — the lane
// still reads its first column — and every sample in a window after Wt has k >= t — its second column; only window Wt itself
// can hold samples of both kinds (a "careful" window: every sample fetches from each lane's true column, explicitly).  Windows are
// compared through keys that grow by one per window in march order: key = dsign * window.
constexpr int kColNoEvent = 0x7fffffff;
struct ColEvents {
	// the wave's distinct event keys in march order: lane i of `events` holds the i-th (kColNoEvent beyond the last), so that the march
	// compares the window it issues / consumes with ONE scalar and touches the lanes only where something happens
	int events = kColNoEvent;
	// What a lane needs to know at its events, packed into ONE register for the march (the flips instantiations have to stay at 64
	// VGPRs too): bits 0-11 / 12-23 its event keys + 1024 (0xfff: none; |key| <= 683 + 1 for edges up to 2048), bit 24 / 25 set =
	// the step to its second column crosses a block edge, bit 28 / 29 set = the column index goes up.  The byte delta to the second
	// column: +-16 (+-64 along v) inside a block, +-(block stride - 3 * 16) (- 3 * 64) across a block edge.
	uint32_t flipinfo = 0x00ffffffu;
	bool ok = true;                     // false: more events than lanes or keys out of range — cannot happen with <= 64 rows and columns per wave; marched per lane if it does
};
__device__ __forceinline__ void col_sort_events(int key_u, int key_v, const ColWave &w, ColEvents &e) {
	const uint32_t lane_i = col_lane_id();
	int last = (int) 0x80000000, count = 0;
	#pragma nounroll
	for (; count < 64; count++) {
		int cand = key_u > last ? key_u : kColNoEvent;
		if (key_v > last && key_v < cand) cand = key_v;
		#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) { const int other = __shfl_xor(cand, d, 64); cand = other < cand ? other : cand; }
		cand = (int) rfl((uint32_t) cand);
		if (cand == kColNoEvent) break;
		e.events = lane_i == (uint32_t) count ? cand : e.events;
		last = cand;
	}
	e.ok = count < 64;
	const uint32_t pu = key_u == kColNoEvent ? 0xfffu : (uint32_t) (key_u + 1024) & 0xfffu, pv = key_v == kColNoEvent ? 0xfffu : (uint32_t) (key_v + 1024) & 0xfffu;
	const bool up_u = w.cu1 > w.cu0, up_v = w.cv1 > w.cv0;
	const bool cross_u = ((uint32_t) w.cu0 & kColEdgeMask) == (up_u ? kColEdgeMask : 0u), cross_v = ((uint32_t) w.cv0 & kColEdgeMask) == (up_v ? kColEdgeMask : 0u);
	e.flipinfo = pu | (pv << 12) | (cross_u ? 1u << 24 : 0u) | (cross_v ? 1u << 25 : 0u) | (up_u ? 1u << 28 : 0u) | (up_v ? 1u << 29 : 0u);
	e.ok = e.ok && __builtin_amdgcn_ballot_w64((key_u != kColNoEvent && (key_u < -1023 || key_u > 1023)) || (key_v != kColNoEvent && (key_v < -1023 || key_v > 1023))) == 0ull;
}
// byte delta to their second column for the lanes that flip in the event window `event` (0 for the others): integer arithmetic
// only (no lane masks: they would cost scalar registers in every window step); CELLS = cells per window of the copy
template <int M, uint32_t CELLS>
__device__ __forceinline__ uint32_t col_event_delta(uint32_t flipinfo, int event) {
	ColConstArgs q = col_dense_args();
	const uint32_t qdim_u = M == 0 ? q->dim_y : q->dim_x, qdim_m = M == 0 ? q->dim_x : (M == 1 ? q->dim_y : q->dim_z);
	const uint32_t stride_u32 = col_windows(qdim_m, CELLS) * kColBlockBytes, stride_v32 = col_blocks(qdim_u) * stride_u32;      // < 2^28 (checked through du64 / dv64 for every lane that flips)
	const uint32_t want = (uint32_t) (event + 1024) & 0xfffu;
	const uint32_t hit_u = (uint32_t) ((int) (((flipinfo ^ want) & 0xfffu) - 1u) >> 31), hit_v = (uint32_t) ((int) ((((flipinfo >> 12) ^ want) & 0xfffu) - 1u) >> 31);   // all ones where the key matches
	const uint32_t mag_u = kColWindowBytes + ((flipinfo >> 24) & 1u) * (stride_u32 - kColRowBytes), mag_v = kColRowBytes + ((flipinfo >> 25) & 1u) * (stride_v32 - kColBlockBytes);
	const uint32_t neg_u = ((flipinfo >> 28) & 1u) - 1u, neg_v = ((flipinfo >> 29) & 1u) - 1u;             // all ones = the column index goes down
	return (((mag_u ^ neg_u) - neg_u) & hit_u) + (((mag_v ^ neg_v) - neg_v) & hit_v);                      // two's complement deltas: the 32-bit sums wrap back into range
}
// The issue frontier of the window gathers, DEPTH windows ahead of the window being consumed.  FLIPS: `vo` follows it — when it passes an
// event window, the lanes that flip there move on to their second column — and `careful` tells whether the window now consumed is one.
template <int M, uint32_t CELLS, int DEPTH, bool FLIPS>
struct ColFrontier {
	uint32_t vo;                        // this lane's column, as a byte offset of the scalar base (biased by 2^30)
	int woff;                           // byte offset, inside a block's run of windows, of the window being ISSUED (may leave 0 .. nw * 256: see col_window_budget)
	int issue_key, issue_at, issue_event, cons_at, cons_event;
	__device__ __forceinline__ void start(uint32_t voff0, int cur, int dsign, const ColEvents &e) {
		vo = voff0; woff = cur * (int) kColBlockBytes;
		issue_key = dsign * cur; issue_at = 0; issue_event = FLIPS ? __builtin_amdgcn_readlane(e.events, 0) : kColNoEvent;
		cons_at = 0; cons_event = issue_event;
	}
	__device__ __forceinline__ void issue(u32x4 &dst, const RayKernelArgs &a, uint64_t s_base, int dsign, const ColEvents &e) {
		if (FLIPS) {
			while (issue_key > issue_event) {                            // (rare: a handful of events per ray)
				vo += col_event_delta<M, CELLS>(e.flipinfo, issue_event);
				issue_at++;
				issue_event = __builtin_amdgcn_readlane(e.events, issue_at & 63);
			}
			issue_key++;
		}
		const uint32_t lane_offset = vo + (uint32_t) woff;                // 2^30 - 2^28 - padding < lane_offset < 2^30 + 2^29: an unsigned 32-bit offset of the one scalar base
#if defined(VR_BOUNDS_CHECK)           // debug build: the address is held against the copy (incl. its padding) and redirected if it leaves it
		managed_load128(dst, VR_BC_ADDRESS(a, s_base + lane_offset, 16u));
#else
		managed_load128_s(dst, lane_offset, s_base);
#endif
		woff += dsign * (int) kColBlockBytes;
	}
	__device__ __forceinline__ bool careful(const ColEvents &e) {      // call once per window step, after its issue
		if (!FLIPS) return false;
		const int key = issue_key - (DEPTH + 1);                          // = dsign * cur: the issue frontier is DEPTH windows ahead and has just moved on
		while (key > cons_event) { cons_at++; cons_event = __builtin_amdgcn_readlane(e.events, cons_at & 63); }
		return key == cons_event;
	}
};

// One TRILINEAR sample at `k` whose element pair is (w0, w1): the general kernel's body from the transparency test on.  B = the
// texel-space ray's offset (coordinate = fma(k, A, B), A from the argument segment); shade_corners(copy, ds, dh, sx, sy, sz, l0, l1)
// fetches the element pair of the shading sample — the one thing that depends on the copy.  PAIR_COPY: that fetch reads the quad-element
// windows of the same axis beside the kernel's own copy; it is then handed their base (RayKernelArgs::alt_copy) and window count
// (col_shade.nwq, in dh.nw) instead of the kernel's, out of the same grouped scalar loads.
template <int SAMPLING, int M, bool PAIR_COPY = false, class ShadeCorners>
__device__ __forceinline__ void col_tri_sample(const RayKernelArgs &a, uint32_t w0, uint32_t w1, float k, const f3 &B, ColRay &ray, uint64_t &live, f4 &acc,
                                               const f4 (&tf_l)[VR_TF_SIZE + 1], const f4 (&dtf_l)[VR_TF_SIZE + 1], const f4 (&org_l)[512], ShadeCorners shade_corners) {
	constexpr bool kQ8 = SAMPLING == VR_SAMPLE_TRILINEAR_Q8;
	if ((__builtin_amdgcn_uicmp((w0 | w1) & a.skip_mask, a.skip_cmp, kIcmpNE) & live) != 0ull && VR_OPEN_LANES(acc.w, live) != 0ull) {
		ColConstArgs q = col_dense_args();
		// everything this sample needs from the argument segment in ONE scalar load (held: the compiler would otherwise load each value
		// where it is first used, one scalar-cache round trip after the other on a path that is a dependent chain)
		RayKernelArgs::ColDenseSample ds;
		ds.ax = q->col_sample.ax; ds.ay = q->col_sample.ay; ds.az = q->col_sample.az; ds.tf_scale = q->col_sample.tf_scale;
		ds.max_x = q->col_sample.max_x; ds.max_y = q->col_sample.max_y; ds.max_z = q->col_sample.max_z; ds.tf_zero_below = q->col_sample.tf_zero_below;
		ds.light_kd = q->col_sample.light_kd; ds.ray_threshold = q->col_sample.ray_threshold;
		hold_scalars(ds.ax, ds.ay, ds.az, ds.tf_scale, ds.max_x, ds.max_y, ds.max_z, ds.tf_zero_below, ds.light_kd, ds.ray_threshold);
		live &= __builtin_amdgcn_fcmpf(k, ray.ky, kFcmpOLE);                                          // the sample's own segment test
		const float xb = VR_FMA(k, ds.ax, B.x), yb = VR_FMA(k, ds.ay, B.y), zb = VR_FMA(k, ds.az, B.z);
		const float raw = col_resolve<M, kQ8>(w0, w1, ds.max_x, ds.max_y, ds.max_z, xb, yb, zb);     // GPURenderer4.cu:76
		const float tb = __builtin_amdgcn_fmed3f(VR_FMA(raw, ds.tf_scale, -0.5f), 0.0f, (float) (VR_TF_SIZE - 1));
		if ((__builtin_amdgcn_fcmpf(tb, ds.tf_zero_below, kFcmpOGE) & live) != 0ull) {
			f4 c;
			{
				const uint32_t i = (uint32_t) (int) tb;
				const float w = filter_weight<kQ8>(__builtin_amdgcn_fractf(tb));
				const f4 c0 = tf_l[i], dc = dtf_l[i];
				c.x = VR_FMA(w, dc.x, c0.x); c.y = VR_FMA(w, dc.y, c0.y); c.z = VR_FMA(w, dc.z, c0.z); c.w = VR_FMA(w, dc.w, c0.w);
			}
			const uint64_t shaded = ds.light_kd > 0.01f ? (__builtin_amdgcn_fcmpf(c.w, 0.05f, kFcmpOGT) & live) : 0ull;   // GPURenderer4.cu:78
			if (shaded != 0ull) {                                                                  // GPURenderer4.cu:41-51 shade_texture
				const f3 org = col_origin_again(org_l, ray.org_slot);                              // (its LDS read is in flight with the scalar load below)
				RayKernelArgs::ColDenseShade dh;                                                   // (one scalar load again)
				for (int i = 0; i < 3; i++) { dh.dir[i] = q->col_shade.dir[i]; dh.light[i] = q->col_shade.light[i]; dh.lh[i] = q->col_shade.lh[i]; }
				dh.kd_scaled = q->col_shade.kd_scaled; dh.nbu = q->col_shade.nbu; dh.nw = PAIR_COPY ? q->col_shade.nwq : q->col_shade.nw;
				const uint8_t *const copy_p = PAIR_COPY ? (const uint8_t *) (uintptr_t) q->alt_copy : ((ColConstKernelArguments) q)->copy;
				hold_scalars(dh.dir[0], dh.dir[1], dh.dir[2], dh.kd_scaled, dh.light[0], dh.light[1], dh.light[2], dh.lh[0], dh.lh[1], dh.lh[2]);
				hold_scalars(dh.nbu, dh.nw, (uint64_t) (uintptr_t) copy_p);
				const f3 p3 = march_point<SAMPLING>(org, mk3(dh.dir[0], dh.dir[1], dh.dir[2]), k);
				const f3 d = mk3(dh.light[0] - p3.x, dh.light[1] - p3.y, dh.light[2] - p3.z);
				const float inv = rsqrt_nr(VR_FMA(d.z, d.z, VR_FMA(d.y, d.y, d.x * d.x)));
				const float sx = VR_FMA(d.x * inv, dh.lh[0], xb), sy = VR_FMA(d.y * inv, dh.lh[1], yb), sz = VR_FMA(d.z * inv, dh.lh[2], zb);
				uint32_t l0, l1;
				shade_corners(copy_p, ds, dh, sx, sy, sz, l0, l1);
				const float raw_l = col_resolve<M, kQ8>(l0, l1, ds.max_x, ds.max_y, ds.max_z, sx, sy, sz);
				const float diffuse = select_lanes(shaded, (raw_l - raw) * dh.kd_scaled);
				c.x += diffuse; c.y += diffuse; c.z += diffuse;
			}
			const float t = select_lanes(live, 1 - acc.w);
			acc.x = VR_FMA(c.x, t, acc.x); acc.y = VR_FMA(c.y, t, acc.y); acc.z = VR_FMA(c.z, t, acc.z); acc.w = VR_FMA(c.w, t, acc.w);
			live &= ~__builtin_amdgcn_fcmpf(acc.w, ds.ray_threshold, kFcmpOGT);                    // ERT (CPURenderer.cpp:35-36)
		}
	}
}

// the end of a march: nothing is in flight into registers the kernel releases (`more`: what else it gathered into)
template <int N, class... More>
__device__ __forceinline__ void col_drain(u32x4 (&slot)[N], More &...more) {
	static_for<0, N>([&](auto j) { pin(slot[j.value]); });
	if constexpr (sizeof...(More) != 0) pin(more...);
	managed_wait<0>();
	static_for<0, N>([&](auto j) { pin(slot[j.value]); });
	if constexpr (sizeof...(More) != 0) pin(more...);
}
// RaycasterBase.h:44-50 write_color.  What the store needs is read off two vector registers the march keeps anyway (lane masks held
// across it would cost scalar registers): a lane has a segment iff its ky is positive (lanes without one were given -1), and is inside
// the buffer iff it has an index
__device__ __forceinline__ void col_store(const ColRay &ray, const f4 &acc) {
	uint32_t ky_bits = __float_as_uint(ray.ky), out_index = ray.out_index;
	pin(ky_bits, out_index);
	uint32_t rgba = 0;
	if (__uint_as_float(ky_bits) > 0.0f) rgba = map_float_int(acc.x, 256) | (map_float_int(acc.y, 256) << 8) | (map_float_int(acc.z, 256) << 16) | (map_float_int(acc.w, 256) << 24);
	if (out_index != 0xffffffffu) ((ColConstKernelArguments) col_dense_args())->out[out_index] = rgba;
}

// ---- colmarch_kernel: TRILINEAR over the quad-element windows ---------------------------------------------------------------------
//
// FLIPS: the instantiation that follows lanes through a change of their cell column (views whose direction carries rounding noise
// in its lateral components); without it (lateral components exactly 0: no lane can flip — the host decides) a wave that does flip
// marches per lane.  Two kernels rather than two loops in one: each stays inside 64 VGPRs / 80 SGPRs without spilling.
template <int SAMPLING, int M, bool FLIPS>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(VR_COL_WAVES, 8)))       // 8 waves per SIMD wanted (64 VGPRs, 80 SGPRs), never by spilling: tests/test_abi.py checks the built kernels
void colmarch_kernel(const RayKernelArgs a, const uint8_t *__restrict__ copy, const float *__restrict__ tf_g, uint32_t *__restrict__ out) {
	constexpr int U = M == 0 ? 1 : 0, V = M == 2 ? 1 : 2;
	__shared__ f4 tf_l[VR_TF_SIZE + 1], dtf_l[VR_TF_SIZE + 1];
	__shared__ f4 org_l[512];                                           // every thread's ray origin (see col_origin_again)
	stage_tf_with_deltas(tf_l, dtf_l, tf_g);
	__syncthreads();
	ColRay ray;
	col_ray_setup(a, org_l, ray);
	if (ray.alive_mask == 0ull) { if (ray.in_frame) out[ray.out_index] = 0u; return; }

	// texel-space ray (oracle/vr_oracle.c axis_setup): coordinate = fma(k, A, B); A is wave-uniform (orthogonal view)
	const f3 A = mk3(uni(ray.dir.x * a.half_x), uni(ray.dir.y * a.half_y), uni(ray.dir.z * a.half_z));
	const f3 B = mk3(VR_FMA(ray.origin.x, a.half_x, a.off_x), VR_FMA(ray.origin.y, a.half_y, a.off_y), VR_FMA(ray.origin.z, a.half_z, a.off_z));
	const float Am = comp3<M>(A), Au = comp3<U>(A), Av = comp3<V>(A);
	const float Bm = comp3<M>(B), Bu = comp3<U>(B), Bv = comp3<V>(B);
	const uint32_t dim_u = U == 0 ? a.dim_x : a.dim_y, dim_m = M == 0 ? a.dim_x : (M == 1 ? a.dim_y : a.dim_z);
	const float max_u = U == 0 ? a.max_x : a.max_y, max_v = V == 1 ? a.max_y : a.max_z;
	const uint32_t nbu = col_blocks(dim_u), nw = col_windows(dim_m);
	const uint64_t stride_u = (uint64_t) nw * kColBlockBytes, stride_v = (uint64_t) nbu * stride_u;       // bytes between lateral blocks

	f4 acc; acc.x = acc.y = acc.z = acc.w = 0.0f;
	uint64_t live = ray.alive_mask;
	float k = ray.kx;                               // the sample being processed (wave-uniform on the column path, per lane on the fallback)

	auto coords = [&](ColConstArgs q, float kk, float &xb, float &yb, float &zb) {          // fma(k, A, B) with A = direction * N/2 (col_sample: the same fp32 products, formed by the host)
		xb = VR_FMA(kk, q->col_sample.ax, B.x); yb = VR_FMA(kk, q->col_sample.ay, B.y); zb = VR_FMA(kk, q->col_sample.az, B.z);
	};
	// the element pair of the sample at kk, from each lane's true column, as a MANAGED gather (the compiler does not see it: a load it knows
	// to be in flight across the window loop's back edge makes it put s_waitcnt vmcnt(0) in front of every window gather, and the prefetch
	// pipeline is gone): wait with managed_wait<>() before use
	auto fetch_at_managed = [&](float kk, uint64_t &both) {
		ColConstArgs q = col_dense_args();
		float xb, yb, zb;
		coords(q, kk, xb, yb, zb);
		managed_load64(both, (uint64_t) (uintptr_t) col_pair_address<M>(a, ((ColConstKernelArguments) q)->copy, q->col_sample.max_x, q->col_sample.max_y, q->col_sample.max_z, q->col_shade.nbu, q->col_shade.nw, xb, yb, zb));
	};
	auto sample = [&](uint32_t w0, uint32_t w1) {                          // the shading sample's pair: one 8-byte load
		col_tri_sample<SAMPLING, M>(a, w0, w1, k, B, ray, live, acc, tf_l, dtf_l, org_l,
			[&](const uint8_t *copy_p, const RayKernelArgs::ColDenseSample &ds, const RayKernelArgs::ColDenseShade &dh, float sx, float sy, float sz, uint32_t &l0, uint32_t &l1) {
				const uint2 both = *(const uint2 *) col_pair_address<M>(a, copy_p, ds.max_x, ds.max_y, ds.max_z, dh.nbu, dh.nw, sx, sy, sz);
				l0 = both.x; l1 = both.y;
			});
	};

	// -- can this wave take the column path?
	auto cell = [&](float kk, float Ac, float Bc, float maxc) { return (int) __builtin_amdgcn_fmed3f(VR_FMA(kk, Ac, Bc), 0.0f, maxc); };
	auto cell_u = [&](float kk) { return cell(kk, Au, Bu, max_u); };
	auto cell_v = [&](float kk) { return cell(kk, Av, Bv, max_v); };
	ColWave wv;
	col_wave_eligibility(ray, Bm, __builtin_fabsf(Am) * ray.step, cell_u, cell_v, wv);      // (advance: a window holds at most ~200 samples)
	int64_t ref, rel0;
	const bool ok = col_lane_offsets(wv, stride_u, stride_v, ref, rel0) && wv.ok;
	const float Bm_l = wv.cm_l;

	const bool has_flips = (wv.flips_u | wv.flips_v) != 0ull;
	// per-lane march with explicit fetches (exact, pipelined: col_lane_march): the few waves that straddle two kx values, and forced testing
	auto per_lane_march = [&]() {
		col_lane_march<kColLaneDepth, uint64_t>(k, ray.step, ray.ky, live,
			[&](float kk, uint64_t &both) { fetch_at_managed(kk, both); },
			[&](uint64_t both) { sample((uint32_t) both, (uint32_t) (both >> 32)); });
	};
	bool lane_march = !ok;
	if (ok) {
		const uint32_t voff0 = (uint32_t) (rel0 + (1ll << 30));
		const uint64_t s_base = col_scalar_base(copy, ref);
		const int dsign = (__float_as_uint(comp3<M>(ray.dir)) >> 31) != 0u ? -1 : 1;     // march direction along m, from the kernel argument's bits: stays scalar
		// window index = floor(cell / 3), also for the cells below 0 a ray reaches after its exit (biased by a multiple of 3; a cell index
		// must never stick to a window: the loops below end when the samples have moved on)
		auto window_of = [](int lc) { return (int) (__umulhi((uint32_t) lc + 0x30000000u, 0xAAAAAAABu) >> 1) - 0x10000000; };
		auto cell_window = [&](float kk) { return window_of((int) VR_FMA(kk, Am, Bm_l)); };      // (cell by truncation)
		int key_u = kColNoEvent, key_v = kColNoEvent;
		if (FLIPS && wv.flips_u != 0ull) key_u = wv.cu0 != wv.cu1 ? dsign * cell_window(__uint_as_float(col_bisect(ray, wv.cu0 != wv.cu1, wv.cu0, cell_u))) : kColNoEvent;
		if (FLIPS && wv.flips_v != 0ull) key_v = wv.cv0 != wv.cv1 ? dsign * cell_window(__uint_as_float(col_bisect(ray, wv.cv0 != wv.cv1, wv.cv0, cell_v))) : kColNoEvent;
		ColEvents ev;
		if (FLIPS && has_flips) col_sort_events(key_u, key_v, wv, ev);

		ColBatch batch = { 0.0f, wv.kx_l, 0 };
		auto next_batch = [&]() { batch.refill(ray.step, col_lane_id(), cell_window); };
		next_batch();
		int pos = 0;                                                        // next sample of the batch
		int cur = col_first_window(batch, nw);                              // the window being consumed
		int guard = col_window_budget(dsign, nw, cur, kColSlots);
		if (!ev.ok || (has_flips && !FLIPS)) lane_march = true;
		else {
			ColFrontier<M, kColCells, kColDepth, FLIPS> front;
			front.start(voff0, cur, dsign, ev);
			u32x4 slot[kColSlots];
			slot[kColSlots - 1] = (u32x4) (0u);
			static_for<0, kColDepth>([&](auto j) { front.issue(slot[j.value], a, s_base, dsign, ev); });
			auto window_step = [&](auto jc) {
				constexpr int c = decltype(jc)::value, n = (c + kColDepth) % kColSlots;
				front.issue(slot[n], a, s_base, dsign, ev);
				__builtin_amdgcn_sched_barrier(0);
				pin(slot[c]); managed_wait<kColDepth>(); pin(slot[c]);
				const u32x4 o = slot[c];
				if (c == 0) live &= __builtin_amdgcn_fcmpf(rlane(batch.kvec, pos), ray.ky, kFcmpOLE);      // lazy exit test: once per rotation of the slots (and by every sample that composites)
				const bool careful = front.careful(ev);                     // an event window: some lane changes its column somewhere inside
				const uint32_t all4 = (o.x | o.y | o.z | o.w) & a.skip_mask;
				bool dense = careful;
				if ((__builtin_amdgcn_uicmp(all4, a.skip_cmp, kIcmpNE) & live) != 0ull) dense = dense || VR_OPEN_LANES(acc.w, live) != 0ull;
				if (!dense) col_skip_window(batch, pos, cur, (int) kColCells + 2, next_batch);
				else {
					const uint32_t first = (uint32_t) (cur * 3);
					col_for_window_samples(batch, pos, cur, (int) kColCells + 2, next_batch, [&](float kk) {
						k = kk;
						if (FLIPS && careful) {
							// from each lane's true column, explicitly (one exposed memory round trip per sample: a few windows per ray)
							uint64_t both;
							fetch_at_managed(k, both);
							pin(both); managed_wait<0>(); pin(both);               // (also the window gathers in flight: a careful window is rare)
							sample((uint32_t) both, (uint32_t) (both >> 32));
						} else {
							const uint32_t sub = rfl((uint32_t) (int) VR_FMA(k, Am, Bm_l)) - first;        // the sample's cell inside the window (the batch keeps only its window)
							sample(sub == 0u ? o.x : (sub == 1u ? o.y : o.z), sub == 0u ? o.y : (sub == 1u ? o.z : o.w));
						}
					});
				}
				cur += dsign;
			};
			while (live != 0ull && guard > 0) {
				static_for<0, kColSlots>(window_step);
				guard -= kColSlots;
			}
			col_drain(slot);
		}
	}
	if (lane_march) per_lane_march();                                   // (one call site: its inlined body is DEPTH + 1 samples long)
	col_store(ray, acc);
}

// ---- the column march for NEAREST sampling (round 4) — the mode that is bit-exact against the reference's own CPURenderer ------------
//
// The same march with Model::sample_data's arithmetic (ModelBase.h:17-23, CPURenderer.cpp:17,24,38): position =
// origin + direction * k (two roundings), cell = map_float_int((position + 1) / 2, dim).  A sample needs ONE voxel, so a window is 16
// consecutive voxels of the lane's column (vr_device.h kColVoxCells): one gather and one transparency test per SIXTEEN samples, and the
// copy is 1 byte per voxel.  The cell along m is tracked UNclamped (a clamped index would stick to the last window and the window loops
// rely on the samples moving on), except for the one value Nm that map_float_int folds onto Nm - 1 for positions on the far face.
__device__ __forceinline__ void managed_load8_at(uint32_t &dst, uint64_t address) {       // zero-extended byte by 64-bit address
	asm volatile("global_load_ubyte %0, %1, off" : "=&v"(dst) : "v"(address));
}

template <int M, bool FLIPS>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(VR_COL_WAVES, 8)))
void colmarch_nearest_kernel(const RayKernelArgs a, const uint8_t *__restrict__ copy, const float *__restrict__ tf_g, uint32_t *__restrict__ out) {
	constexpr int U = M == 0 ? 1 : 0, V = M == 2 ? 1 : 2;
	constexpr int kCells = (int) kColVoxCells;
	__shared__ f4 tf_l[VR_TF_SIZE];
	__shared__ float unit_l[256];                                       // unit[s] = (float) s / 255.0f, the quotient Raycaster::shade forms twice per shaded sample
	__shared__ f4 org_l[512];                                           // every thread's ray origin
	{
		const uint32_t t = threadIdx.x;
		if (t < VR_TF_SIZE) tf_l[t] = ((const f4 *) tf_g)[t];
		if (t < 256u) unit_l[t] = (float) t / 255.0f;
	}
	__syncthreads();
	ColRay ray;
	col_ray_setup(a, org_l, ray);
	if (ray.alive_mask == 0ull) { if (ray.in_frame) out[ray.out_index] = 0u; return; }

	const float dm = comp3<M>(ray.dir), du = comp3<U>(ray.dir), dv = comp3<V>(ray.dir);            // kernel arguments: scalar
	const float om = comp3<M>(ray.origin), ou = comp3<U>(ray.origin), ov = comp3<V>(ray.origin);
	const uint32_t dim_u = U == 0 ? a.dim_x : a.dim_y, dim_v = V == 1 ? a.dim_y : a.dim_z, dim_m = M == 0 ? a.dim_x : (M == 1 ? a.dim_y : a.dim_z);
	const float half_m = M == 0 ? a.half_x : (M == 1 ? a.half_y : a.half_z);
	const uint32_t nbu = col_blocks(dim_u), nw = col_windows(dim_m, kColVoxCells);
	const uint64_t stride_u = (uint64_t) nw * kColBlockBytes, stride_v = (uint64_t) nbu * stride_u;

	f4 acc; acc.x = acc.y = acc.z = acc.w = 0.0f;
	uint64_t live = ray.alive_mask;
	float k = ray.kx;
	// transfer_fn[sample / TF_RATIO] (CPURenderer.cpp:31) is (0,0,0,0) for sample <= opaque_above; the per-WINDOW test is the weaker
	// "every voxel below the largest power of two <= opaque_above + 1" (a mask on the packed bytes; windows that fail it test per sample)
	const int opaque_above = ((int) a.tf_zero_below + 1) * VR_TF_RATIO - 1;
	uint32_t near_mask = 0u, near_cmp = 1u;                             // nothing may be skipped: 0 != 1 always
	if (opaque_above >= 0) { const uint32_t p2 = 1u << (31 - __builtin_clz((uint32_t) opaque_above + 1u)); near_mask = (0xffu & ~(p2 - 1u)) * 0x01010101u; near_cmp = 0u; }

	// address of the voxel Model::sample_data reads for a position (every index clamped: any position is in bounds); dims, lateral blocks
	// and windows per column as the caller holds them
	auto voxel_address = [&](const uint8_t *copy_p, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t blocks_u, uint32_t windows, f3 pos) {
		const uint32_t ix = map_float_int((pos.x + 1) * 0.5f, nx), iy = map_float_int((pos.y + 1) * 0.5f, ny), iz = map_float_int((pos.z + 1) * 0.5f, nz);
		const uint32_t iu = U == 0 ? ix : iy, iv = V == 1 ? iy : iz, im = M == 0 ? ix : (M == 1 ? iy : iz);
		const uint32_t block = col_lateral_block(iu, iv, blocks_u) * windows + (im >> 4);
		const uint32_t in_block = col_in_block(iu, iv) + (im & 15u);      // < 256: summed in 32 bits
		const uint8_t *p = copy_p + ((uint64_t) block * kColBlockBytes + in_block);
		return VR_BC_POINTER(a, const uint8_t *, p, 1u);
	};
	auto voxel_address_at = [&](ColConstArgs q, f3 pos) {                 // ... with everything from the argument segment
		const uint32_t qdim_u = U == 0 ? q->dim_x : q->dim_y, qdim_m = M == 0 ? q->dim_x : (M == 1 ? q->dim_y : q->dim_z);
		return voxel_address(((ColConstKernelArguments) q)->copy, q->dim_x, q->dim_y, q->dim_z, col_blocks(qdim_u), col_windows(qdim_m, kColVoxCells), pos);
	};
	auto position = [&](ColConstArgs q, float kk) {                      // CPURenderer.cpp:17,24,38: origin + direction * k, two roundings per axis
		const f3 o = col_origin_again(org_l, ray.org_slot);
		return mk3(o.x + q->p.view.direction[0] * kk, o.y + q->p.view.direction[1] * kk, o.z + q->p.view.direction[2] * kk);
	};
	// one sample at `k` whose voxel is s: the general kernel's NEAREST body from the transparency test on (CPURenderer.cpp:29-39) — the
	// reference's unfused arithmetic, NOT col_tri_sample's
	auto sample = [&](uint32_t s) {
		if ((__builtin_amdgcn_sicmp((int) s, opaque_above, kIcmpSGT) & live) != 0ull && VR_OPEN_LANES(acc.w, live) != 0ull) {
			ColConstArgs q = col_dense_args();
			live &= __builtin_amdgcn_fcmpf(k, ray.ky, kFcmpOLE);
			uint32_t idx = s / VR_TF_RATIO;
			asm volatile("" : "+v"(idx));
			f4 cur = tf_l[idx & (VR_TF_SIZE - 1u)];
			const float kd = q->col_sample.light_kd, threshold = q->col_sample.ray_threshold;      // (adjacent: one scalar load)
			hold_scalars(kd, threshold);
			const uint64_t shaded = kd > 0.01f ? (__builtin_amdgcn_fcmpf(cur.w, 0.05f, kFcmpOGT) & live) : 0ull;
			if (shaded != 0ull) {                                                             // RaycasterBase.h:87-98 shade
				// everything the shading needs from the argument segment in ONE scalar load (see col_tri_sample), beside the LDS read of the origin
				const f3 o = col_origin_again(org_l, ray.org_slot);
				RayKernelArgs::ColDenseShade dh;
				for (int i = 0; i < 3; i++) { dh.dir[i] = q->col_shade.dir[i]; dh.light[i] = q->col_shade.light[i]; dh.dim[i] = q->col_shade.dim[i]; }
				dh.nbu = q->col_shade.nbu; dh.nw = q->col_shade.nw;
				const uint8_t *const copy_p = ((ColConstKernelArguments) q)->copy;
				hold_scalars(dh.dir[0], dh.dir[1], dh.dir[2], dh.light[0], dh.light[1], dh.light[2], dh.dim[0], dh.dim[1], dh.dim[2], dh.nbu, dh.nw, (uint64_t) (uintptr_t) copy_p);
				const f3 pt = mk3(o.x + dh.dir[0] * k, o.y + dh.dir[1] * k, o.z + dh.dir[2] * k);        // position(q, k)
				const f3 d = mk3(dh.light[0] - pt.x, dh.light[1] - pt.y, dh.light[2] - pt.z);
				const float inv = 1.0f / __builtin_sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
				const f3 l = mk3(d.x * inv, d.y * inv, d.z * inv);
				const f3 ps = mk3(pt.x + l.x * 0.01f, pt.y + l.y * 0.01f, pt.z + l.z * 0.01f);
				const uint32_t s_l = *voxel_address(copy_p, dh.dim[0], dh.dim[1], dh.dim[2], dh.nbu, dh.nw, ps);      // (the constants held above)
				const float sl = unit_l[s_l], sc = unit_l[s & 255u];                          // RaycasterBase.h:93-96
				const float diffuse = select_lanes(shaded, (sl - sc) * kd);
				cur.x += diffuse; cur.y += diffuse; cur.z += diffuse;
			}
			const float t = select_lanes(live, 1 - acc.w);                                    // CPURenderer.cpp:34
			acc.x = acc.x + cur.x * t; acc.y = acc.y + cur.y * t;
			acc.z = acc.z + cur.z * t; acc.w = acc.w + cur.w * t;
			live &= ~__builtin_amdgcn_fcmpf(acc.w, threshold, kFcmpOGT);                      // CPURenderer.cpp:35-36
		}
	};

	// -- can this wave take the column path?  (the coordinate along m that the lanes must share: the origin's component)
	auto cell_lat = [&](float kk, float oc, float dc, uint32_t n) { return (int) map_float_int(((oc + dc * kk) + 1) * 0.5f, n); };
	auto cell_u = [&](float kk) { return cell_lat(kk, ou, du, dim_u); };
	auto cell_v = [&](float kk) { return cell_lat(kk, ov, dv, dim_v); };
	ColWave wv;
	col_wave_eligibility(ray, om, __builtin_fabsf(dm * half_m) * ray.step, cell_u, cell_v, wv);
	int64_t ref, rel0;
	const bool ok = col_lane_offsets(wv, stride_u, stride_v, ref, rel0) && wv.ok;
	const float om_l = wv.cm_l;
	// the cell along m of the wave's sample at kk: map_float_int's product by truncation, NOT clamped, but for the value Nm (positions on
	// the far face, folded onto Nm - 1 like map_float_int does)
	auto cell_m = [&](float kk) { const int c = (int) (((om_l + dm * kk) + 1.0f) * half_m); return c == (int) dim_m ? (int) dim_m - 1 : c; };
	const bool has_flips = (wv.flips_u | wv.flips_v) != 0ull;
	auto per_lane_march = [&]() {                                        // exact, pipelined (col_lane_march): waves that straddle two kx values, forced testing
		col_lane_march<kColLaneDepth, uint32_t>(k, ray.step, ray.ky, live,
			[&](float kk, uint32_t &s) { ColConstArgs q = col_dense_args(); managed_load8_at(s, (uint64_t) (uintptr_t) voxel_address_at(q, position(q, kk))); },
			[&](uint32_t s) { sample(s); });
	};
	bool lane_march = !ok;
	if (ok) {
		const uint32_t voff0 = (uint32_t) (rel0 + (1ll << 30));
		const uint64_t s_base = col_scalar_base(copy, ref);
		const int dsign = (__float_as_uint(dm) >> 31) != 0u ? -1 : 1;
		auto cell_window = [&](float kk) { return cell_m(kk) >> 4; };      // floor(cell / 16), also below 0
		int key_u = kColNoEvent, key_v = kColNoEvent;
		if (FLIPS && wv.flips_u != 0ull) key_u = wv.cu0 != wv.cu1 ? dsign * cell_window(__uint_as_float(col_bisect(ray, wv.cu0 != wv.cu1, wv.cu0, cell_u))) : kColNoEvent;
		if (FLIPS && wv.flips_v != 0ull) key_v = wv.cv0 != wv.cv1 ? dsign * cell_window(__uint_as_float(col_bisect(ray, wv.cv0 != wv.cv1, wv.cv0, cell_v))) : kColNoEvent;
		ColEvents ev;
		if (FLIPS && has_flips) col_sort_events(key_u, key_v, wv, ev);

		ColBatch batch = { 0.0f, wv.kx_l, 0 };
		auto next_batch = [&]() { batch.refill(ray.step, col_lane_id(), cell_window); };
		next_batch();
		int pos = 0;
		int cur = col_first_window(batch, nw);
		int guard = col_window_budget(dsign, nw, cur, kColSlots);
		if (!ev.ok || (has_flips && !FLIPS)) lane_march = true;
		else {
			ColFrontier<M, kColVoxCells, kColDepth, FLIPS> front;
			front.start(voff0, cur, dsign, ev);
			u32x4 slot[kColSlots];
			slot[kColSlots - 1] = (u32x4) (0u);
			static_for<0, kColDepth>([&](auto j) { front.issue(slot[j.value], a, s_base, dsign, ev); });
			auto window_step = [&](auto jc) {
				constexpr int c = decltype(jc)::value, n = (c + kColDepth) % kColSlots;
				front.issue(slot[n], a, s_base, dsign, ev);
				__builtin_amdgcn_sched_barrier(0);
				pin(slot[c]); managed_wait<kColDepth>(); pin(slot[c]);
				const u32x4 o = slot[c];
				if (c == 0) live &= __builtin_amdgcn_fcmpf(rlane(batch.kvec, pos), ray.ky, kFcmpOLE);
				const bool careful = front.careful(ev);
				const uint32_t all16 = (o.x | o.y | o.z | o.w) & near_mask;
				bool dense = careful;
				if ((__builtin_amdgcn_uicmp(all16, near_cmp, kIcmpNE) & live) != 0ull) dense = dense || VR_OPEN_LANES(acc.w, live) != 0ull;
				if (!dense) col_skip_window(batch, pos, cur, kCells + 2, next_batch);
				else {
					const int first = cur * kCells;
					col_for_window_samples(batch, pos, cur, kCells + 2, next_batch, [&](float kk) {
						k = kk;
						if (FLIPS && careful) {                            // the voxel of each lane's true column, explicitly
							ColConstArgs q = col_dense_args();
							uint32_t s;
							managed_load8_at(s, (uint64_t) (uintptr_t) voxel_address_at(q, position(q, k)));
							pin(s); managed_wait<0>(); pin(s);
							sample(s);
						} else {
							const uint32_t sub = (uint32_t) ((int) rfl((uint32_t) cell_m(k)) - first) & 15u;      // the sample's voxel inside the window (uniform)
							const uint32_t word = (sub >> 2) == 0u ? o.x : ((sub >> 2) == 1u ? o.y : ((sub >> 2) == 2u ? o.z : o.w));
							sample((word >> ((sub & 3u) * 8u)) & 0xffu);
						}
					});
				}
				cur += dsign;
			};
			while (live != 0ull && guard > 0) {
				static_for<0, kColSlots>(window_step);
				guard -= kColSlots;
			}
			col_drain(slot);
		}
	}
	if (lane_march) per_lane_march();                                   // (one call site: its inlined body is DEPTH + 1 samples long)
	col_store(ray, acc);
}

// ---- the TRILINEAR column march over the 1-byte voxel windows (voxcol_tri_kernel) ---------------------------------------------------
//
// colmarch_kernel's views, colmarch_kernel's arithmetic, colmarch_nearest_kernel's copy (kCopyColVox*: 16 consecutive voxels of a column
// per 16-byte window, 1 byte per voxel instead of the 16/3 of the quad-element windows).  On these views every lane of a wave samples the
// same cell along m at every step and stays in one cell column (but for at most one flip per lateral axis), so a wave needs only the
// RECTANGLE of columns its lanes sample: their own, their +1 neighbours and the columns they flip to (at most 7 x 7 at 0.5 cells per
// pixel; the host admits a frame only when its 8 x 8-pixel waves fit in 64 columns, the kernel re-checks per wave).  Lane j gathers the
// window of column j of that rectangle (ONE managed 16-byte gather per lane and 16 cells); a sample's eight corners come from the four
// lanes that own its 2 x 2 columns — each owner aligns the two slices of the wave-uniform cell into one dword, four ds_bpermute and four
// v_perm rebuild the quad-element pair (w0, w1) that colmarch_kernel reads from its copy, and from there on the sample is col_tri_sample.
// The aligned dword holds four slices, so ONE exchange serves the samples of three consecutive cells (a cell group, window_step).
// A flip is a switch of the lane's owner index at the first k of its second column (col_bisect),
// exact per sample: no event windows.  The transparency test is ONE per window and wave: the slices 16w .. 16w + 16 of every column of
// the rectangle (the 16 cells of window w need the first slice of window w + 1 too).  Waves that cannot share the k sequence or the
// rectangle march per lane with explicit byte loads from the same copy; the shading sample is an explicit fetch of its 2 x 2 x 2 corners.
// PAIRS (voxcol_pairs_kernel): both explicit fetches — the shading sample's and the per-lane march's — read the element pair of the
// position from the QUAD-ELEMENT windows of the same axis instead (col_pair_address: one 8-byte load, as colmarch_kernel; base in
// RayKernelArgs::alt_copy, window count in col_shade.nwq).  The march itself streams the voxel windows as before.  The same values, so
// the same image; the host launches it for lit frames when that copy can be had (vr_hip_api.cpp launch_frame).
// prefetch depth in windows of 16 cells (the window after the one consumed has landed too: it holds the last cell's second slice)
#ifndef VR_VOXCOL_DEPTH
#define VR_VOXCOL_DEPTH 3
#endif
#ifndef VR_VOXCOL_WAVES
#define VR_VOXCOL_WAVES VR_COL_WAVES
#endif
constexpr int kVoxColDepth = VR_VOXCOL_DEPTH, kVoxColSlots = kVoxColDepth + 1;
static_assert(kVoxColDepth >= 2 && 2 * kVoxColSlots + kVoxColDepth + 4 <= 64, "kColPadBytes");

template <int SAMPLING, int M, bool FLIPS, bool PAIRS>
__device__ __forceinline__ void voxcol_march(const RayKernelArgs &a, const uint8_t *__restrict__ copy, const float *__restrict__ tf_g, uint32_t *__restrict__ out,
                                             f4 (&tf_l)[VR_TF_SIZE + 1], f4 (&dtf_l)[VR_TF_SIZE + 1], f4 (&org_l)[512]) {
	constexpr int U = M == 0 ? 1 : 0, V = M == 2 ? 1 : 2;
	constexpr int kCells = (int) kColVoxCells;
	stage_tf_with_deltas(tf_l, dtf_l, tf_g);
	__syncthreads();
	ColRay ray;
	col_ray_setup(a, org_l, ray);
	if (ray.alive_mask == 0ull) { if (ray.in_frame) out[ray.out_index] = 0u; return; }

	const f3 A = mk3(uni(ray.dir.x * a.half_x), uni(ray.dir.y * a.half_y), uni(ray.dir.z * a.half_z));
	const f3 B = mk3(VR_FMA(ray.origin.x, a.half_x, a.off_x), VR_FMA(ray.origin.y, a.half_y, a.off_y), VR_FMA(ray.origin.z, a.half_z, a.off_z));
	const float Am = comp3<M>(A), Au = comp3<U>(A), Av = comp3<V>(A);
	const float Bm = comp3<M>(B), Bu = comp3<U>(B), Bv = comp3<V>(B);
	const uint32_t dim_u = U == 0 ? a.dim_x : a.dim_y, dim_v = V == 1 ? a.dim_y : a.dim_z, dim_m = M == 0 ? a.dim_x : (M == 1 ? a.dim_y : a.dim_z);
	const float max_u = U == 0 ? a.max_x : a.max_y, max_v = V == 1 ? a.max_y : a.max_z;
	const uint32_t nbu = col_blocks(dim_u), nw = col_windows(dim_m, kColVoxCells);
	const uint64_t stride_u = (uint64_t) nw * kColBlockBytes, stride_v = (uint64_t) nbu * stride_u;

	f4 acc; acc.x = acc.y = acc.z = acc.w = 0.0f;
	uint64_t live = ray.alive_mask;
	float k = ray.kx;

	// the eight corner voxels of a texel-space position as the quad-element pair (march index i, i + 1), by explicit byte loads from the
	// voxel windows; every index clamped (at the upper faces like the quad copy: the weight there is exactly 0): any position is in bounds.
	// PAIRS: the pair itself, one 8-byte load from the quad-element windows (copy_p / windows are then that copy's)
	auto corners_at = [&](const uint8_t *copy_p, float mx, float my, float mz, uint32_t blocks_u, uint32_t windows, float xb, float yb, float zb,
	                      uint32_t &w0, uint32_t &w1) {
		if constexpr (PAIRS) {
			const uint2 both = *(const uint2 *) col_pair_address<M>(a, copy_p, mx, my, mz, blocks_u, windows, xb, yb, zb);
			w0 = both.x; w1 = both.y;
			return;
		}
		const uint32_t ix = (uint32_t) (int) __builtin_amdgcn_fmed3f(xb, 0.0f, mx), iy = (uint32_t) (int) __builtin_amdgcn_fmed3f(yb, 0.0f, my),
		               iz = (uint32_t) (int) __builtin_amdgcn_fmed3f(zb, 0.0f, mz);
		const float fu = U == 0 ? mx : my, fv = V == 1 ? my : mz, fm = M == 0 ? mx : (M == 1 ? my : mz);
		const uint32_t iu = U == 0 ? ix : iy, iv = V == 1 ? iy : iz, im = M == 0 ? ix : (M == 1 ? iy : iz);
		const uint32_t iu1 = iu + ((float) iu < fu ? 1u : 0u), iv1 = iv + ((float) iv < fv ? 1u : 0u), im1 = im + ((float) im < fm ? 1u : 0u);
		// 32-bit byte offsets from the copy's start (the host takes this kernel only for copies below 4 GiB): one VGPR per address
		auto along = [](uint32_t m) { return (m >> 4) * kColBlockBytes + (m & 15u); };
		auto ld = [&](uint32_t off) { return (uint32_t) *VR_BC_POINTER(a, const uint8_t *, copy_p + off, 1u); };
		const uint32_t l00 = col_lateral_offset(iu, iv, blocks_u, windows), l10 = col_lateral_offset(iu1, iv, blocks_u, windows),
		               l01 = col_lateral_offset(iu, iv1, blocks_u, windows), l11 = col_lateral_offset(iu1, iv1, blocks_u, windows), m0 = along(im), m1 = along(im1);
		w0 = ld(l00 + m0) | (ld(l10 + m0) << 8) | (ld(l01 + m0) << 16) | (ld(l11 + m0) << 24);
		w1 = ld(l00 + m1) | (ld(l10 + m1) << 8) | (ld(l01 + m1) << 16) | (ld(l11 + m1) << 24);
	};
	auto fetch_at = [&](float kk, uint32_t &w0, uint32_t &w1) {         // the corners of the sample at kk, from each lane's true column
		ColConstArgs q = col_dense_args();
		const float xb = VR_FMA(kk, q->col_sample.ax, B.x), yb = VR_FMA(kk, q->col_sample.ay, B.y), zb = VR_FMA(kk, q->col_sample.az, B.z);
		corners_at(PAIRS ? (const uint8_t *) (uintptr_t) q->alt_copy : ((ColConstKernelArguments) q)->copy, q->col_sample.max_x, q->col_sample.max_y, q->col_sample.max_z,
		           q->col_shade.nbu, PAIRS ? q->col_shade.nwq : q->col_shade.nw, xb, yb, zb, w0, w1);
	};
	auto sample = [&](uint32_t w0, uint32_t w1) {                          // the shading sample's pair: eight byte loads (PAIRS: one 8-byte load)
		col_tri_sample<SAMPLING, M, PAIRS>(a, w0, w1, k, B, ray, live, acc, tf_l, dtf_l, org_l,
			[&](const uint8_t *copy_p, const RayKernelArgs::ColDenseSample &ds, const RayKernelArgs::ColDenseShade &dh, float sx, float sy, float sz, uint32_t &l0, uint32_t &l1) {
				corners_at(copy_p, ds.max_x, ds.max_y, ds.max_z, dh.nbu, dh.nw, sx, sy, sz, l0, l1);
			});
	};

	// -- can this wave take the column path?  (the shared conditions, and a column rectangle of at most 64 columns)
	auto cell = [&](float kk, float Ac, float Bc, float maxc) { return (int) __builtin_amdgcn_fmed3f(VR_FMA(kk, Ac, Bc), 0.0f, maxc); };
	auto cell_u = [&](float kk) { return cell(kk, Au, Bu, max_u); };
	auto cell_v = [&](float kk) { return cell(kk, Av, Bv, max_v); };
	ColWave wv;
	col_wave_eligibility(ray, Bm, __builtin_fabsf(Am) * ray.step, cell_u, cell_v, wv);
	const float Bm_l = wv.cm_l;
	const int cu0 = wv.cu0, cu1 = wv.cu1, cv0 = wv.cv0, cv1 = wv.cv1;
	const uint64_t flips = wv.flips_u | wv.flips_v;
	bool ok = wv.ok && (FLIPS || flips == 0ull);
	// the rectangle [ru0, ru1] x [rv0, rv1]: every column a lane samples, with its +1 neighbours
	int ru0 = cu0 < cu1 ? cu0 : cu1, ru1 = (cu0 > cu1 ? cu0 : cu1) + 1, rv0 = cv0 < cv1 ? cv0 : cv1, rv1 = (cv0 > cv1 ? cv0 : cv1) + 1;
	#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		const int a0 = __shfl_xor(ru0, d, 64), a1 = __shfl_xor(ru1, d, 64), a2 = __shfl_xor(rv0, d, 64), a3 = __shfl_xor(rv1, d, 64);
		ru0 = a0 < ru0 ? a0 : ru0; ru1 = a1 > ru1 ? a1 : ru1; rv0 = a2 < rv0 ? a2 : rv0; rv1 = a3 > rv1 ? a3 : rv1;
	}
	ru0 = (int) rfl((uint32_t) ru0); ru1 = (int) rfl((uint32_t) ru1); rv0 = (int) rfl((uint32_t) rv0); rv1 = (int) rfl((uint32_t) rv1);
	const int rw = ru1 - ru0 + 1, nrect = rw * (rv1 - rv0 + 1);
	ok = ok && nrect <= 64;
	// the column this lane OWNS (gathers for the wave): column j of the rectangle, row by row; lanes beyond it repeat the last one; indices
	// clamped at the upper faces.  Offsets relative to the rectangle's first column, biased by 2^30 (col_scalar_base)
	const uint32_t lane_i = col_lane_id();
	int own_u, own_v;
	{
		const int j = (int) lane_i < nrect ? (int) lane_i : nrect - 1;
		const int jv = j / rw;
		own_u = ru0 + (j - jv * rw); own_v = rv0 + jv;
		own_u = own_u < (int) dim_u - 1 ? own_u : (int) dim_u - 1; own_v = own_v < (int) dim_v - 1 ? own_v : (int) dim_v - 1;
	}
	const int64_t ref = (int64_t) col_lateral_offset64((uint32_t) ru0, (uint32_t) rv0, stride_u, stride_v);
	const int64_t rel = (int64_t) col_lateral_offset64((uint32_t) own_u, (uint32_t) own_v, stride_u, stride_v) - ref;
	ok = ok && __builtin_amdgcn_ballot_w64(rel < 0 || rel >= (1ll << 28)) == 0ull;

	// exact: waves that straddle two kx values, or too many columns.  PAIRS: pipelined (col_lane_march), the element pair as one managed
	// 8-byte load.  Without PAIRS (vr_hip_set_column_copy(2)) a sample is eight byte loads: 8 (DEPTH + 1) slot registers (40 at
	// depth 4) beside the ~30 a sample keeps live are past the 64 VGPRs of these kernels, so that body stays unpipelined
	auto per_lane_march = [&]() {
		if constexpr (PAIRS) {
			col_lane_march<kColLaneDepth, uint64_t>(k, ray.step, ray.ky, live,
				[&](float kk, uint64_t &both) {
					ColConstArgs q = col_dense_args();
					const float xb = VR_FMA(kk, q->col_sample.ax, B.x), yb = VR_FMA(kk, q->col_sample.ay, B.y), zb = VR_FMA(kk, q->col_sample.az, B.z);
					managed_load64(both, (uint64_t) (uintptr_t) col_pair_address<M>(a, (const uint8_t *) (uintptr_t) q->alt_copy, q->col_sample.max_x, q->col_sample.max_y, q->col_sample.max_z,
					                                                                q->col_shade.nbu, q->col_shade.nwq, xb, yb, zb));
				},
				[&](uint64_t both) { sample((uint32_t) both, (uint32_t) (both >> 32)); });
			return;
		}
		while (live != 0ull) {
			uint32_t w0, w1;
			fetch_at(k, w0, w1);
			sample(w0, w1);
			k += ray.step;
			live &= __builtin_amdgcn_fcmpf(k, ray.ky, kFcmpOLE);
		}
	};
	if (ok) {
		const uint32_t voff = (uint32_t) (rel + (1ll << 30));
		const uint64_t s_base = col_scalar_base(copy, ref);
		const int dsign = (__float_as_uint(comp3<M>(ray.dir)) >> 31) != 0u ? -1 : 1;
		const bool forward = dsign > 0;
		// where this lane reads its corners: the byte address (ds_bpermute) of the owner of its (u, v) column; the owners of (u+1, v), (u, v+1)
		// and (u+1, v+1) follow at +4, +4 rw, +4 rw + 4.  A lane whose column flips switches at the first k of its second column
		// (col_bisect; the cell is monotone in k): samples with k >= t read the second column — exact per sample.  The switch is made where
		// the corners are exchanged (window_step): `at` moves on and the threshold is spent, and between two switches the march compares k
		// with ONE scalar, t_next = the bits of the smallest threshold no lane has spent yet (0: unordered as bits — look at every sample)
		const uint32_t rw4 = (uint32_t) rw * 4u;
		uint32_t at = (uint32_t) ((cu0 - ru0) + (cv0 - rv0) * rw) * 4u;
		float t_u = __builtin_inff(), t_v = __builtin_inff();
		uint32_t step_u = 0u, step_v = 0u;
		auto next_threshold = [&]() {
			const float t = t_u < t_v ? t_u : t_v;
			uint32_t m = t > 0.0f ? __float_as_uint(t) : 0u;                // (positive floats order like their bits)
			// (ds_swizzle: the partner lane is part of the instruction — a shuffle's address registers would be kept across the whole march)
			static_for<0, 5>([&](auto j) { const uint32_t other = (uint32_t) __builtin_amdgcn_ds_swizzle((int) m, ((1 << decltype(j)::value) << 10) | 0x1f); m = other < m ? other : m; });
			const uint32_t h0 = (uint32_t) __builtin_amdgcn_readlane((int) m, 0), h1 = (uint32_t) __builtin_amdgcn_readlane((int) m, 32);
			return h0 < h1 ? h0 : h1;
		};
		uint32_t t_next = 0x7f800000u;
		if (FLIPS && flips != 0ull) {
			const uint32_t bu = col_bisect(ray, cu0 != cu1, cu0, cell_u), bv = col_bisect(ray, cv0 != cv1, cv0, cell_v);
			t_u = cu0 != cu1 ? __uint_as_float(bu) : __builtin_inff();
			t_v = cv0 != cv1 ? __uint_as_float(bv) : __builtin_inff();
			step_u = (uint32_t) (cu1 - cu0) * 4u; step_v = (uint32_t) (cv1 - cv0) * rw4;      // (two's complement: the sums wrap back into range)
			t_next = next_threshold();
		}
		auto cell_window = [&](float kk) { return (int) VR_FMA(kk, Am, Bm_l) >> 4; };      // (cell by truncation, as colmarch_kernel)
		ColBatch batch = { 0.0f, wv.kx_l, 0 };
		auto next_batch = [&]() { batch.refill(ray.step, lane_i, cell_window); };
		next_batch();
		int pos = 0;
		int cur = col_first_window(batch, nw);
		// what lies beyond a column's windows is a neighbouring block's or the zeroed padding
		int guard = col_window_budget(dsign, nw, cur, kVoxColSlots);
		const ColEvents no_events;
		ColFrontier<M, kColVoxCells, kVoxColDepth, false> front;
		front.start(voff, cur, dsign, no_events);
		// the first slice of window cur + 1 — the last cell of window cur needs it: marching up it is the next window's (in a slot), marching
		// down the previous one's, kept in `carry` (for the first window: one extra gather, oldest of the pipeline)
		uint32_t carry;
		{
			const uint32_t lane_offset = voff + (uint32_t) ((cur + 1) * (int) kColBlockBytes);
#if defined(VR_BOUNDS_CHECK)
			asm volatile("global_load_dword %0, %1, off" : "=&v"(carry) : "v"(VR_BC_ADDRESS(a, s_base + lane_offset, 4u)));
#else
			managed_load32(carry, lane_offset, (const void *) (uintptr_t) s_base);
#endif
		}
		u32x4 slot[kVoxColSlots];
		slot[kVoxColSlots - 1] = (u32x4) (0u);
		static_for<0, kVoxColDepth>([&](auto j) { front.issue(slot[j.value], a, s_base, dsign, no_events); });
		auto window_step = [&](auto jc) {
			constexpr int c = decltype(jc)::value, n = (c + kVoxColDepth) % kVoxColSlots, c1 = (c + 1) % kVoxColSlots;
			front.issue(slot[n], a, s_base, dsign, no_events);
			__builtin_amdgcn_sched_barrier(0);
			pin(slot[c]); pin(slot[c1]); pin(carry); managed_wait<kVoxColDepth - 1>(); pin(slot[c]); pin(slot[c1]); pin(carry);
			const u32x4 o = slot[c];
			const uint32_t nx = forward ? slot[c1].x : carry;
			// (held as scalars: left to the compiler, their copies at the window's branch go through a vector register, and such a copy may
			// name a gather still in flight — tests/test_voxcol_march.py walks the built code)
			pos = (int) rfl((uint32_t) pos); cur = (int) rfl((uint32_t) cur);
			if (c == 0) live &= __builtin_amdgcn_fcmpf(rlane(batch.kvec, pos), ray.ky, kFcmpOLE);
			const uint32_t all17 = (o.x | o.y | o.z | o.w | (nx & 0xffu)) & a.skip_mask;
			// dense: some column of the rectangle holds a voxel at or above the skip threshold in slices 16 cur .. 16 cur + 16, and a lane is open
			const bool dense = (__builtin_amdgcn_ballot_w64(lane_i < (uint32_t) nrect && all17 != a.skip_cmp) != 0ull) & (VR_OPEN_LANES(acc.w, live) != 0ull);
			if (!dense) col_skip_window(batch, pos, cur, kCells + 2, next_batch);
			else {
				const int first = cur * kCells;
				// One corner exchange per CELL GROUP.  The dword an owner aligns at cell `base` holds the four slices base .. base + 3 of its
				// column, i.e. the cells base, base + 1 and base + 2; a sample advances at most one cell, so the samples that follow read their
				// pair out of the four exchanged dwords with another v_perm selector (sub - base: uniform) for as long as their cell stays in the
				// group and no lane has changed its owner.  Marching down the group ends at the sample's cell instead (base = sub - 2, not below
				// the window's first cell).  A new window always exchanges again: `o` and `nx` are other registers then.
				// voxcol_tri_kernel with FLIPS has no room for the four dwords beside its thresholds and steps (it is at 63 - 64 VGPRs without them; the
				// other eighteen kernels hold them in 60 - 64): there a group holds the owner's aligned dword alone (one register) and every sample
				// exchanges it; the selects, the alignment and the owner switch are still made once per group.
				constexpr bool kHoldCorners = !FLIPS || PAIRS;
				int base = 64;
				uint32_t group = 0u, p00 = 0u, p10 = 0u, p01 = 0u, p11 = 0u;
				auto exchange = [&]() {
					p00 = (uint32_t) __builtin_amdgcn_ds_bpermute((int) at, (int) group); p10 = (uint32_t) __builtin_amdgcn_ds_bpermute((int) (at + 4u), (int) group);
					p01 = (uint32_t) __builtin_amdgcn_ds_bpermute((int) (at + rw4), (int) group); p11 = (uint32_t) __builtin_amdgcn_ds_bpermute((int) (at + rw4 + 4u), (int) group);
				};
				// the cells of the batch's 64 samples, once per window and batch (cell_window's own arithmetic): a sample reads its cell with one
				// v_readlane instead of forming it again from three scalars
				int cells = (int) VR_FMA(batch.kvec, Am, Bm_l);
				auto next_cells = [&]() { next_batch(); cells = (int) VR_FMA(batch.kvec, Am, Bm_l); };
				col_for_window_samples(batch, pos, cur, kCells + 2, next_cells, [&](float kk, int lane) {
					k = kk;
					const int sub = (__builtin_amdgcn_readlane(cells, lane) - first) & 15;              // the sample's cell inside the window (uniform)
					const bool passed = FLIPS && __float_as_uint(kk) >= t_next;                         // some lane is at its second column from this sample on
					if ((uint32_t) (sub - base) > 2u || passed) {
						base = forward ? sub : (sub > 2 ? sub - 2 : 0);
						const uint32_t qw = (uint32_t) base >> 2;
						const uint32_t lo = qw == 0u ? o.x : (qw == 1u ? o.y : (qw == 2u ? o.z : o.w));
						const uint32_t hi = qw == 0u ? o.y : (qw == 1u ? o.z : (qw == 2u ? o.w : nx));
						group = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t) base & 3u);                  // byte i: slice base + i
						if (FLIPS && passed) {
							// t is monotone in k: a threshold that was passed is spent (+inf), and the wave waits for the smallest one left
							const bool pu = k >= t_u, pv = k >= t_v;
							at += (pu ? step_u : 0u) + (pv ? step_v : 0u);
							t_u = pu ? __builtin_inff() : t_u; t_v = pv ? __builtin_inff() : t_v;
							t_next = next_threshold();
						}
						if constexpr (kHoldCorners) exchange();
					}
					if constexpr (!kHoldCorners) exchange();
					// (u,v) (u+1,v) (u,v+1) (u+1,v+1) of slice sub -> w0, of slice sub + 1 -> w1: bytes sub - base and sub - base + 1 of the four dwords
					const uint32_t sel = 0x05010400u + (uint32_t) (sub - base) * 0x01010101u;
					const uint32_t t0 = __builtin_amdgcn_perm(p10, p00, sel), t1 = __builtin_amdgcn_perm(p11, p01, sel);
					sample(__builtin_amdgcn_perm(t1, t0, 0x05040100u), __builtin_amdgcn_perm(t1, t0, 0x07060302u));
				});
			}
			carry = o.x;
			cur += dsign;
		};
		while (live != 0ull && guard > 0) {
			static_for<0, kVoxColSlots>(window_step);
			guard -= kVoxColSlots;
		}
		col_drain(slot, carry);
	} else per_lane_march();
	col_store(ray, acc);
}

template <int SAMPLING, int M, bool FLIPS>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(VR_VOXCOL_WAVES, 8)))       // 64 VGPRs, 80 SGPRs, no spills: tests/test_voxcol_march.py
void voxcol_tri_kernel(const RayKernelArgs a, const uint8_t *__restrict__ copy, const float *__restrict__ tf_g, uint32_t *__restrict__ out) {
	__shared__ f4 tf_l[VR_TF_SIZE + 1], dtf_l[VR_TF_SIZE + 1];
	__shared__ f4 org_l[512];
	voxcol_march<SAMPLING, M, FLIPS, false>(a, copy, tf_g, out, tf_l, dtf_l, org_l);
}
// ... shading from the quad-element windows at a.alt_copy (PAIRS): tests/test_voxcol_pairs.py holds these twelve to the same limits
template <int SAMPLING, int M, bool FLIPS>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(VR_VOXCOL_WAVES, 8)))
void voxcol_pairs_kernel(const RayKernelArgs a, const uint8_t *__restrict__ copy, const float *__restrict__ tf_g, uint32_t *__restrict__ out) {
	__shared__ f4 tf_l[VR_TF_SIZE + 1], dtf_l[VR_TF_SIZE + 1];
	__shared__ f4 org_l[512];
	voxcol_march<SAMPLING, M, FLIPS, true>(a, copy, tf_g, out, tf_l, dtf_l, org_l);
}

// One frame of the column kernels: an orthogonal view along args.col_axis, full march, 1-byte voxels; `copy` = the column windows
// args.layout names (kLayoutColumn / kLayoutVoxCol).  launch_raymarch hands such a frame over (launch_frame chooses the layout).
hipError_t launch_colmarch(const RayKernelArgs &args, const void *copy, const float *tf, void *out, hipStream_t stream) {
	if (args.clip_on) return hipErrorInvalidValue;           // the column kernels march the whole cube: launch_frame takes none for a clipped frame
	RayKernelArgs a = args;
	tile_grid(a.p.out_width, a.p.out_rows, a.phase_x, a.phase_y, 512u, a.tiles_x, a.tiles_y);
	const dim3 grid(a.tiles_x * a.tiles_y), block(512);
	auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, stream, a, (const uint8_t *) copy, tf, (uint32_t *) out); };
	// lateral direction components exactly 0: no lane can change its column — the kernel without the flip logic
	const uint32_t m = a.col_axis;
	const bool flips = a.p.view.direction[m == 0u ? 1 : 0] != 0.0f || a.p.view.direction[m == 2u ? 1 : 2] != 0.0f;
	const bool voxels = a.layout == kLayoutVoxCol;                      // TRILINEAR over the voxel windows (kCopyColVoxX ..): voxcol_tri_kernel
	const bool pairs = voxels && a.alt_copy != 0ull;                    // ... shading from the quad-element windows at alt_copy: voxcol_pairs_kernel
	dispatch_axis_flag(m, flips, [&](auto axis, auto flag) {
		constexpr int AX = decltype(axis)::value;
		constexpr bool FL = decltype(flag)::value;
		constexpr int T = VR_SAMPLE_TRILINEAR, Q8 = VR_SAMPLE_TRILINEAR_Q8;
		if (a.p.sampling == VR_SAMPLE_NEAREST) go(colmarch_nearest_kernel<AX, FL>);      // voxel windows (kCopyColVoxX ..)
		else if (a.p.sampling == VR_SAMPLE_TRILINEAR_Q8) { if (pairs) go(voxcol_pairs_kernel<Q8, AX, FL>); else if (voxels) go(voxcol_tri_kernel<Q8, AX, FL>); else go(colmarch_kernel<Q8, AX, FL>); }
		else if (pairs) go(voxcol_pairs_kernel<T, AX, FL>); else if (voxels) go(voxcol_tri_kernel<T, AX, FL>); else go(colmarch_kernel<T, AX, FL>);
	});
	return hipGetLastError();
}

}  // namespace vr
