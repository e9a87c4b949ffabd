// vr_march.h — what the gfx950 (CDNA4) kernel units of the volume raycaster share: vector and LDS types, the volume fetch, the per-ray
// helpers, table staging, and the selector of the instantiation a frame runs.  Private to the kernel units (vr_raymarch.hip,
// vr_project.hip, vr_kernels.hip, vr_schedule.hip, vr_builders.hip); host files include only vr_device.h.  Written for MI355X only.
//
// The hot path: per-pixel ray generation, cube intersection, empty-space leaping, ray-march with NEAREST or manual
// TRILINEAR sampling of a volume held in linear HBM, transfer-function lookup from an LDS-staged table, optional
// diffuse shading, front-to-back compositing with a wavefront-ballot early-ray-termination test, RGBA8 store.
// What it computes is the reference's render_ray (CPURenderer.cpp:11-41 for NEAREST, GPURenderer4.cu:53-87 for
// TRILINEAR); how it is laid out is not:
//   * one 64-lane wavefront owns one 8x8-pixel screen tile; a workgroup is 8 waves = 32x16 pixels (16 waves = 32x32 for the
//     64-bit address tables) and stages one copy of the tables per workgroup;
//   * the transfer function (+ per-entry deltas for the filtered lookup), the ESL bit-volume and per-axis address tables live in LDS;
//   * liveness is one scalar 64-bit wave mask updated with v_cmp results; the loop runs while it is non-zero (the wave's vote);
//   * workgroup id = tile number inside 8x8-tile blocks: every block is spread over all eight XCDs (plain interleave — measured
//     faster than one screen region per XCD, see the tile-map comment in the kernel);
//   * the frame clear is fused: every pixel of the output is written exactly once (misses write 0), there is no
//     separate memset pass over the framebuffer (the reference clears first, CPURenderer.cpp:47).
//
// Numerics.  Every unit is compiled with -ffp-contract=off.  NEAREST mode keeps the reference's float operation order
// expression by expression (IEEE divide / sqrt, no fused ops), so its output is bit-identical to the reference's CPU
// renderer.  TRILINEAR mode is defined with explicit fused multiply-adds (oracle/vr_oracle.c states the same sequence).
#pragma once

#include "vr_device.h"
#include <initializer_list>

namespace vr {

#define VR_FMA(a, b, c) __builtin_fmaf((a), (b), (c))

struct f3 { float x, y, z; };
struct f4 { float x, y, z, w; };

__device__ __forceinline__ f3 mk3(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ f3 ld3(const float *p) { return mk3(p[0], p[1], p[2]); }
// common.h:88-96 flmin/flmax — written as the reference's ternaries (NaN behaviour included)
__device__ __forceinline__ float flmin(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float flmax(float a, float b) { return a > b ? a : b; }

// common.h:105-110 map_float_int
__device__ __forceinline__ uint32_t map_float_int(float f, uint32_t n) {
	int i = (int) (f * (float) n);
	if (i >= (int) n) i = (int) n - 1;
	if (i < 0) i = 0;
	return (uint32_t) i;
}

// LDS image, one per workgroup
struct __attribute__((aligned(16))) LdsTables {
	f4 tf[VR_TF_SIZE + 1];         // premultiplied TF; entry 128 duplicates 127 (clamp addressing of the filtered lookup)
	f4 dtf[VR_TF_SIZE + 1];        // dtf[i] = tf[i+1] - tf[i] (same fp32 subtraction the lerp would do per sample)
	uint32_t esl[VR_ESL_VOLUME_SIZE];
	float unit[256];               // NEAREST, 1-byte voxels: unit[s] = (float) s / 255.0f, the quotient Raycaster::shade forms twice per shaded sample
};

// How voxel addresses are formed (template parameter ADDR):
//   kAddr32   : 32-bit BYTE offsets from a scalar base (global_load ... v_off, s[base:base+1]); brick copy <= 4 GiB, dims <=
//               1024; per-axis offset tables in LDS, 512-thread workgroups (8 waves = 32x16 pixels)
//   kAddrLut64: dims <= 2048 and any size (BASELINE config 5: 2048^3 u16 = 64 GiB of bricks): the z table holds 64-bit byte
//               offsets, x and y 32-bit offsets inside one brick slab; 1024-thread workgroups (16 waves = 32x32 pixels) so
//               that two workgroups per CU still reach the 32-wave limit next to 56 KiB of tables each
//   kAddrWide : full 64-bit index arithmetic, no tables (anything larger; also the linear layout beyond 4 GiB)
enum : int { kAddr32 = 0, kAddrLut64 = 1, kAddrWide = 2 };


// Brick address tables at FIXED LDS positions, so a lookup is one shift + one ds_read with an immediate offset:
// z entries first ({offset(z), offset(min(z+1, Z-1))} pairs: one ds_read_b64 / b128 serves both slices), then x, then y.
// Every table has kLutPad (vr_device.h) extra entries on both sides that repeat the edge entry (clamp addressing): a speculative
// fetch up to kLutPad cells outside the volume still reads a valid address, so the march needs neither a coordinate clamp nor a
// min(k, ky) per sample (the host checks that kDepth ray steps plus rounding stay below kLutPad cells, else the clamping variant runs).
template <int ADDR> struct LutCfg          { static constexpr uint32_t max_dim = 0,    z_words = 0, x_at = 0,    y_at = 0,     words = 4,     threads = 512; };
template <> struct LutCfg<kAddr32>         { static constexpr uint32_t max_dim = 1024, z_words = 2, x_at = (1024 + 2 * kLutPad) * 2, y_at = x_at + 1024 + 2 * kLutPad,
                                                                       words = y_at + 1024 + 2 * kLutPad, threads = 512; };
template <> struct LutCfg<kAddrLut64>      { static constexpr uint32_t max_dim = 2048, z_words = 4, x_at = (2048 + 2 * kLutPad) * 4, y_at = x_at + 2048 + 2 * kLutPad,
                                                                       words = y_at + 2048 + 2 * kLutPad, threads = 1024; };

template <int BPV> struct VoxelT;
template <> struct VoxelT<1> { typedef uint8_t type; };
template <> struct VoxelT<2> { typedef uint16_t type; };

// ---- bounds-checked debug build (make EXTRA=-DVR_BOUNDS_CHECK; see RayKernelArgs) -----------------------------------------------
#ifdef VR_BOUNDS_CHECK
enum : uint32_t { kBcTableIndex = 1, kBcOffset = 2, kBcAddress = 3, kBcCostSlot = 4 };
__shared__ uint32_t bc_table_entries[3];       // entries of the x / y / z address tables as staged by this workgroup (dim + 2 * kLutPad)
__device__ __forceinline__ void bc_report(const RayKernelArgs &a, uint32_t code, uint64_t value, uint64_t limit) {
	if (atomicCAS(a.bc_fault, 0u, code) == 0u) {
		a.bc_fault[1] = blockIdx.x; a.bc_fault[2] = threadIdx.x; a.bc_fault[3] = (uint32_t) value; a.bc_fault[4] = (uint32_t) (value >> 32); a.bc_fault[5] = (uint32_t) limit;
	}
}
// table index i (cell coordinate, -kLutPad .. dim - 1 + kLutPad) of table `axis` (0 x, 1 y, 2 z as STAGED: the run axis is "z")
__device__ __forceinline__ int bc_index(const RayKernelArgs &a, uint32_t axis, int i) {
	const uint32_t entry = (uint32_t) (i + kLutPad);
	if (entry < bc_table_entries[axis]) return i;
	bc_report(a, kBcTableIndex + (axis << 8), (uint64_t) (int64_t) i, bc_table_entries[axis]);
	return 0;
}
__device__ __forceinline__ uint32_t bc_offset(const RayKernelArgs &a, uint32_t offset, uint32_t bytes) {
	if ((uint64_t) offset + bytes <= a.bc_bytes) return offset;
	bc_report(a, kBcOffset, offset, a.bc_bytes);
	return 0u;
}
__device__ __forceinline__ uint64_t bc_address(const RayKernelArgs &a, uint64_t address, uint32_t bytes) {
	if (address >= a.bc_base && address + bytes <= a.bc_base + a.bc_bytes) return address;
	if (a.alt_copy != 0ull && address >= a.alt_copy && address + bytes <= a.alt_copy + a.bc_alt_bytes) return address;
	bc_report(a, kBcAddress, address, a.bc_bytes);
	return a.bc_base;
}
#define VR_BC_INDEX(a, axis, i) bc_index((a), (axis), (i))
#define VR_BC_OFFSET(a, offset, bytes) bc_offset((a), (offset), (bytes))
#define VR_BC_ADDRESS(a, address, bytes) bc_address((a), (uint64_t) (address), (bytes))
#define VR_BC_POINTER(a, T, pointer, bytes) ((T) (uintptr_t) bc_address((a), (uint64_t) (uintptr_t) (pointer), (bytes)))
#else
#define VR_BC_INDEX(a, axis, i) (i)
#define VR_BC_OFFSET(a, offset, bytes) (offset)
#define VR_BC_ADDRESS(a, address, bytes) (address)
#define VR_BC_POINTER(a, T, pointer, bytes) (pointer)
#endif

// ---- volume fetch --------------------------------------------------------------------------------------------

// "Managed" gathers of the software-pipelined march: issued through inline asm, so the compiler's s_waitcnt insertion does not
// know them and the ray loop waits for exactly the loads it is about to read (s_waitcnt vmcnt(N), N = the loads issued since).
// Left to the compiler, the waits at the loop's control-flow joins are merged conservatively (vmcnt(1) / vmcnt(0) where vmcnt(4)
// would do) and the prefetch distance collapses to one sample — the march then runs at memory latency, not at issue rate.
// Only the hot instantiations use them (1-byte voxels, 32-bit table addressing, the quad or run bricks); the loop drains them
// with s_waitcnt vmcnt(0) before it lets go of the destination registers.
template <int BPV, int ADDR, int LAYOUT> struct Managed {
	static constexpr bool value = BPV == 1 && ADDR == kAddr32 && (is_brick_table_layout(LAYOUT) || is_run_layout(LAYOUT));
};
__device__ __forceinline__ void managed_load32(uint32_t &dst, uint32_t byte_offset, const void *base) {
	asm volatile("global_load_dword %0, %1, %2" : "=v"(dst) : "v"(byte_offset), "s"(base));
}
__device__ __forceinline__ void managed_load8(uint32_t &dst, uint32_t byte_offset, const void *base) {       // zero-extended byte
	asm volatile("global_load_ubyte %0, %1, %2" : "=v"(dst) : "v"(byte_offset), "s"(base));
}
// TRILINEAR with 2-byte voxels: the two 8-byte elements of a quad-brick sample, by 64-bit address (copies beyond 4 GiB included)
template <int BPV, int ADDR, int LAYOUT> struct ManagedTri {
	static constexpr bool value = Managed<BPV, ADDR, LAYOUT>::value || (BPV == 2 && (LAYOUT == kLayoutBricked || LAYOUT == kLayoutOct) && (ADDR == kAddr32 || ADDR == kAddrLut64));
};
__device__ __forceinline__ void managed_load64(uint64_t &dst, uint64_t address) {      // split into halves only AFTER the wait
	asm volatile("global_load_dwordx2 %0, %1, off" : "=&v"(dst) : "v"(address));
}
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void managed_load128(u32x4 &dst, uint64_t address) {        // oct bricks: the 2x2x2 neighbourhood of 2-byte voxels
	asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(dst) : "v"(address));
}

// Single voxel (NEAREST).  LINEAR: the reference's array.  BRICKED: component 0 of the quad element (x,y,z) IS v(x,y,z), so
// NEAREST reads the same Z-ordered bricks as TRILINEAR with one aligned element load and keeps their view-independent
// cache-line footprint; the value — hence the image — is identical.
template <int BPV, int ADDR, int LAYOUT, bool MANAGED = false>
__device__ __forceinline__ uint32_t fetch_voxel(const void *vol, const RayKernelArgs &a, const uint32_t *lut,
                                                int ix, int iy, int iz) {
	typedef typename VoxelT<BPV>::type V;
	if (is_brick_table_layout(LAYOUT)) {
		typedef LutCfg<ADDR> L;                      // table lookups take indices -kLutPad .. dim - 1 + kLutPad
		ix = VR_BC_INDEX(a, 0, ix); iy = VR_BC_INDEX(a, 1, iy); iz = VR_BC_INDEX(a, 2, iz);
		const uint32_t exy = lut[(int) L::x_at + kLutPad + ix] + lut[(int) L::y_at + kLutPad + iy];
		const uint8_t *q;
		constexpr uint32_t kBytes = LAYOUT == kLayoutVoxel ? BPV : 4u;       // what the load below reads
		(void) kBytes;
		if (ADDR == kAddr32) {
			if (MANAGED && Managed<BPV, ADDR, LAYOUT>::value) {
				uint32_t word;
				if (LAYOUT == kLayoutVoxel) managed_load8(word, VR_BC_OFFSET(a, exy + lut[(int) L::z_words * (iz + kLutPad)], kBytes), vol);
				else managed_load32(word, VR_BC_OFFSET(a, exy + lut[(int) L::z_words * (iz + kLutPad)], kBytes), vol);
				return word;
			}
			q = (const uint8_t *) vol + (exy + lut[(int) L::z_words * (iz + kLutPad)]);
		} else {
			const uint2 z = *(const uint2 *) (lut + (int) L::z_words * (iz + kLutPad));
			q = (const uint8_t *) vol + ((((uint64_t) z.y) << 32 | z.x) + exy);
		}
		q = VR_BC_POINTER(a, const uint8_t *, q, kBytes);
		// the RAW element word: the voxel is its low byte / half (voxel_of).  Masking here would hand the compiler an operation on the
		// loaded value that it hoists to the loop latch of the software-pipelined march — behind an s_waitcnt vmcnt(0) that drains
		// every prefetch once per iteration (measured: the NEAREST full march was latency bound because of it).
		if (LAYOUT == kLayoutVoxel) return *(const V *) q;           // voxel bricks: the element IS the voxel
		return *(const uint32_t *) q;
	}
	if (ADDR == kAddrWide) {
		uint64_t idx = ((uint64_t) iz * a.dim_y + iy) * a.dim_x + ix;
		return *VR_BC_POINTER(a, const V *, (const V *) vol + idx, (uint32_t) sizeof(V));
	} else {
		uint32_t idx = (iz * a.dim_y + iy) * a.dim_x + ix;
		return *VR_BC_POINTER(a, const V *, (const V *) vol + idx, (uint32_t) sizeof(V));
	}
}

// the voxel inside what fetch_voxel returned (bricked layouts return the whole quad element)
template <int BPV, int LAYOUT> __device__ __forceinline__ uint32_t voxel_of(uint32_t fetched) {
	return LAYOUT == kLayoutBricked ? (BPV == 1 ? fetched & 0xffu : fetched & 0xffffu) : fetched;
}

// ModelBase.h:17-23 Model::sample_data
template <int BPV, int ADDR, int LAYOUT, bool MANAGED = false>
__device__ __forceinline__ uint32_t sample_nearest(const void *vol, const RayKernelArgs &a, const uint32_t *lut, f3 pos) {
	uint32_t iz = map_float_int((pos.z + 1) * 0.5f, a.dim_z);
	uint32_t iy = map_float_int((pos.y + 1) * 0.5f, a.dim_y);
	uint32_t ix = map_float_int((pos.x + 1) * 0.5f, a.dim_x);
	return fetch_voxel<BPV, ADDR, LAYOUT, MANAGED>(vol, a, lut, (int) ix, (int) iy, (int) iz);
}

// The same voxel for a position INSIDE the cube, or at most kLutPad cells outside it when the layout has (padded) tables:
// truncation alone gives the cell — a fraction above -1 truncates to 0 like the lower clamp, the upper clamp is the repeated
// edge entry of the table — and ((pos + 1) * 0.5f) * n == (pos + 1) * (0.5f * n) bit for bit (both scalings by 0.5 are exact).
template <int BPV, int ADDR, int LAYOUT, bool MANAGED = false>
__device__ __forceinline__ uint32_t sample_nearest_incube(const void *vol, const RayKernelArgs &a, const uint32_t *lut, f3 pos) {
	int iz = (int) ((pos.z + 1) * a.half_z), iy = (int) ((pos.y + 1) * a.half_y), ix = (int) ((pos.x + 1) * a.half_x);
	if (!(is_brick_table_layout(LAYOUT) && ADDR != kAddrWide)) {        // no tables: clamp the index at the upper face
		const int mz = (int) a.dim_z - 1, my = (int) a.dim_y - 1, mx = (int) a.dim_x - 1;
		ix = ix < mx ? ix : mx; iy = iy < my ? iy : my; iz = iz < mz ? iz : mz;
	}
	return fetch_voxel<BPV, ADDR, LAYOUT, MANAGED>(vol, a, lut, ix, iy, iz);
}

// NEAREST in the SCALED domain, for volumes whose edges are powers of two: ps = origin * half + (direction * half) * k, and the
// cell is (int)(ps + half).  Scaling by a power of two commutes with every fp32 rounding of the reference's sequence
// t = dir * k; p = origin + t; q = p + 1; cell = (int)(q * half)   (q * half is exact), so the cell is the same bit for bit while
// one multiplication per axis disappears from the per-sample address chain.
template <int BPV, int ADDR, int LAYOUT, bool MANAGED = false>
__device__ __forceinline__ uint32_t sample_nearest_scaled(const void *vol, const RayKernelArgs &a, const uint32_t *lut, f3 ps) {
	return fetch_voxel<BPV, ADDR, LAYOUT, MANAGED>(vol, a, lut, (int) (ps.x + a.half_x), (int) (ps.y + a.half_y), (int) (ps.z + a.half_z));
}

__device__ __forceinline__ float lerp(float a, float b, float t) { return VR_FMA(t, b - a, a); }

// ---- manual trilinear fetch, split in two so that the ray-march loop can software-pipeline it -----------------------
//
// tri_issue():   texel-space coordinates -> clamp -> cell index + fractions -> address -> ISSUE the loads.
// tri_resolve(): unpack the returned words and do the 7 lerps.
// Semantics = tex3D with normalised coordinates, linear filter, clamp addressing (GPURenderer4.cu:76,136-141).
// Clamping the COORDINATE to [0, N-1] is equivalent to clamping the two neighbour indices: outside that range both
// neighbours clamp to the same voxel and lerp(a, a, t) == a exactly; at N-1 the weight of the upper neighbour is exactly
// 0.  Coordinates are >= 0 after the clamp, so float->int truncation is floor() and v_fract_f32 is x - floor(x).
// Because of the clamp every address is in bounds for ANY coordinate, so loads may be issued speculatively.
template <int BPV, int LAYOUT> struct TriFetch {
	// bricked: slice z quad, slice z+1 quad (u8: one dword each, u16: two dwords each);
	// linear : the four x-pairs (y,z) (y+1,z) (y,z+1) (y+1,z+1)
	uint32_t w0, w1, w2, w3;
	uint64_t q;                                      // run bricks, managed load: both slices as ONE 64-bit destination (w0 = low, w1 = high)
	uint64_t q2;                                     // 2-byte voxels, managed loads: q = the element of slice z (w0, w1), q2 = of slice z+1 (w2, w3)
	u32x4 o;                                         // oct bricks, managed load: the whole 16-byte element (w0 .. w3)
};

// `clamp` (wave-uniform) = false is allowed for positions INSIDE the volume's cube, i.e. coordinates in (-1, N): there
// truncation toward zero already yields the clamped cell (x in (-1, 0) -> 0 like clamp-to-0; x in (N-1, N) -> N-1 like
// clamp-to-N-1), so the three v_med3 are only needed for the interpolation weights, and those are computed in
// tri_resolve, which most samples of a sparse volume never reach (transparent shortcut of the ray loop).
template <int BPV, int ADDR, int LAYOUT, bool MANAGED = false>
__device__ __forceinline__ TriFetch<BPV, LAYOUT> tri_issue(const void *vol, const RayKernelArgs &a, const uint32_t *lut,
                                                           float xb, float yb, float zb, bool clamp) {
	TriFetch<BPV, LAYOUT> f;
	f.q = 0; f.q2 = 0; f.o = (u32x4) (0u);
	if (clamp) {
		xb = __builtin_amdgcn_fmed3f(xb, 0.0f, a.max_x);
		yb = __builtin_amdgcn_fmed3f(yb, 0.0f, a.max_y);
		zb = __builtin_amdgcn_fmed3f(zb, 0.0f, a.max_z);
	}
	int ix = (int) xb, iy = (int) yb, iz = (int) zb;                // table layouts: -kLutPad .. dim - 1 + kLutPad are valid
	if (LAYOUT != kLayoutLinear && ADDR != kAddrWide) {             // (debug build: each index against the table it is about to address)
		const bool run_y = LAYOUT == kLayoutRunY;
		(void) run_y;
		ix = VR_BC_INDEX(a, 0, ix); iy = VR_BC_INDEX(a, run_y ? 2 : 1, iy); iz = VR_BC_INDEX(a, run_y ? 1 : 2, iz);
	}
	f.w0 = f.w1 = f.w2 = f.w3 = 0;
	if (is_run_layout(LAYOUT)) {
		// run bricks: two tables hold the cell column's offset, the third the ABSOLUTE 64-bit address of (brick slab, run coordinate
		// & 7); the two slices along the run axis are 8 adjacent bytes (the ninth element of a run duplicates the next brick's first).
		// kLayoutRun: runs along z, columns (x,y); kLayoutRunY: runs along y, columns (x,z) — the table regions swap roles.
		typedef LutCfg<kAddr32> L;
		const int irun = LAYOUT == kLayoutRunY ? iy : iz, iother = LAYOUT == kLayoutRunY ? iz : iy;
		const uint32_t exy = lut[(int) L::x_at + kLutPad + ix] + lut[(int) L::y_at + kLutPad + iother];
		const uint2 zz = *(const uint2 *) (lut + 2 * (irun + kLutPad));
		const uint64_t address = VR_BC_ADDRESS(a, (((uint64_t) zz.y) << 32 | zz.x) + exy, 8u);
		if (MANAGED && Managed<BPV, ADDR, LAYOUT>::value) {
			managed_load64(f.q, address);
		} else {
			const uint2 both = *(const uint2 *) address;                                     // global_load_dwordx2, 4-byte aligned
			f.w0 = both.x; f.w1 = both.y;
		}
	} else if (LAYOUT == kLayoutOct) {
		// oct bricks (2-byte voxels): ONE aligned 16-byte element holds both slices; tables as for the quad bricks (the z + 1 entry is unused)
		typedef LutCfg<ADDR> L;
		const uint32_t exy = lut[(int) L::x_at + kLutPad + ix] + lut[(int) L::y_at + kLutPad + iy];
		uint64_t address;
		if (ADDR == kAddr32) address = (uint64_t) (uintptr_t) vol + (uint64_t) (exy + lut[(int) L::z_words * (iz + kLutPad)]);
		else { const uint2 zz = *(const uint2 *) (lut + (int) L::z_words * (iz + kLutPad)); address = (uint64_t) (uintptr_t) vol + ((((uint64_t) zz.y) << 32 | zz.x) + exy); }
		address = VR_BC_ADDRESS(a, address, 16u);
		if (MANAGED && ManagedTri<BPV, ADDR, LAYOUT>::value) managed_load128(f.o, address);
		else { const uint4 v = *(const uint4 *) address; f.w0 = v.x; f.w1 = v.y; f.w2 = v.z; f.w3 = v.w; }
	} else if (LAYOUT == kLayoutBricked) {
		constexpr uint32_t kElem = 4 * BPV;
		const uint8_t *q0, *q1;
		if (ADDR == kAddrWide) {
			const uint32_t iz1 = (uint32_t) iz + 1 < a.dim_z ? iz + 1 : iz;
			const uint64_t bxy = (uint64_t) (iy >> 3) * a.nbx + (ix >> 3), slab = (uint64_t) a.nbx * a.nby;
			const uint32_t lxy = brick_spread(BPV, a.brick_plane, 0, ix & 7u) | brick_spread(BPV, a.brick_plane, 1, iy & 7u);
			q0 = (const uint8_t *) vol + (((iz >> 3) * slab + bxy) * kBrickPitch + (lxy | brick_spread(BPV, a.brick_plane, 2, iz & 7u))) * kElem;
			q1 = (const uint8_t *) vol + (((iz1 >> 3) * slab + bxy) * kBrickPitch + (lxy | brick_spread(BPV, a.brick_plane, 2, iz1 & 7u))) * kElem;
		} else {
			// per-axis byte-offset tables in LDS (LutCfg): brick base + Morton-dilated in-brick offset, split by axis
			typedef LutCfg<ADDR> L;
			const uint32_t exy = lut[(int) L::x_at + kLutPad + ix] + lut[(int) L::y_at + kLutPad + iy];
			if (ADDR == kAddr32) {
				const uint2 zz = *(const uint2 *) (lut + (int) L::z_words * (iz + kLutPad));
				q0 = (const uint8_t *) vol + (exy + zz.x);
				q1 = (const uint8_t *) vol + (exy + zz.y);
			} else {
				const uint4 zz = *(const uint4 *) (lut + (int) L::z_words * (iz + kLutPad));
				q0 = (const uint8_t *) vol + ((((uint64_t) zz.y) << 32 | zz.x) + exy);
				q1 = (const uint8_t *) vol + ((((uint64_t) zz.w) << 32 | zz.z) + exy);
			}
		}
		q0 = VR_BC_POINTER(a, const uint8_t *, q0, kElem); q1 = VR_BC_POINTER(a, const uint8_t *, q1, kElem);
		if (BPV == 1 && MANAGED && Managed<BPV, ADDR, LAYOUT>::value) {
			managed_load32(f.w0, (uint32_t) (q0 - (const uint8_t *) vol), vol);
			managed_load32(f.w1, (uint32_t) (q1 - (const uint8_t *) vol), vol);
		} else if (BPV == 1) {                           // 2 x global_load_dword, 4-byte aligned
			f.w0 = *(const uint32_t *) q0;
			f.w1 = *(const uint32_t *) q1;
		} else if (MANAGED && ManagedTri<BPV, ADDR, LAYOUT>::value) {
			managed_load64(f.q, (uint64_t) (uintptr_t) q0);
			managed_load64(f.q2, (uint64_t) (uintptr_t) q1);
		} else {                                         // 2 x global_load_dwordx2, 8-byte aligned
			const uint2 lo = *(const uint2 *) q0, hi = *(const uint2 *) q1;
			f.w0 = lo.x; f.w1 = lo.y; f.w2 = hi.x; f.w3 = hi.y;
		}
	} else {
		// LINEAR layout: one load per x-pair at VOXEL alignment (slow when the address is odd, see vr_device.h)
		const uint8_t *p00, *p10, *p01, *p11;
		if (ADDR == kAddrWide) {
			const uint64_t e = (((uint64_t) iz * a.dim_y + iy) * a.dim_x + ix) * BPV;
			p00 = (const uint8_t *) vol + e;
			p10 = p00 + a.stride_y * BPV; p01 = p00 + a.stride_z * BPV; p11 = p01 + a.stride_y * BPV;
		} else {
			const uint32_t e = ((iz * a.dim_y + iy) * a.dim_x + ix) * (uint32_t) BPV;
			const uint32_t sy = (uint32_t) a.stride_y * BPV, sz = (uint32_t) a.stride_z * BPV;
			p00 = (const uint8_t *) vol + e;
			p10 = (const uint8_t *) vol + (e + sy); p01 = (const uint8_t *) vol + (e + sz); p11 = (const uint8_t *) vol + (e + sz + sy);
		}
		p00 = VR_BC_POINTER(a, const uint8_t *, p00, 2u * BPV); p10 = VR_BC_POINTER(a, const uint8_t *, p10, 2u * BPV);
		p01 = VR_BC_POINTER(a, const uint8_t *, p01, 2u * BPV); p11 = VR_BC_POINTER(a, const uint8_t *, p11, 2u * BPV);
		if (BPV == 1) {
			uint16_t h0, h1, h2, h3;
			__builtin_memcpy(&h0, p00, 2); __builtin_memcpy(&h1, p10, 2); __builtin_memcpy(&h2, p01, 2); __builtin_memcpy(&h3, p11, 2);
			f.w0 = h0; f.w1 = h1; f.w2 = h2; f.w3 = h3;
		} else {
			__builtin_memcpy(&f.w0, p00, 4); __builtin_memcpy(&f.w1, p10, 4); __builtin_memcpy(&f.w2, p01, 4); __builtin_memcpy(&f.w3, p11, 4);
		}
	}
	return f;
}

// returns the interpolated RAW voxel value
// VR_SAMPLE_TRILINEAR_Q8: an interpolation weight in 9-bit fixed point with 8 fractional bits, rint(w * 256) / 256 (v_rndne_f32)
template <bool Q8> __device__ __forceinline__ float filter_weight(float w) {
	return Q8 ? __builtin_rintf(w * 256.0f) * (1.0f / 256.0f) : w;
}

// (xb, yb, zb): the texel-space coordinates the words were fetched at; the fetch slots of the march do not carry them — the few
// samples that get this far recompute them from the sample's k (three fused multiply-adds, the same values bit for bit)
// `along_y` (wave-uniform, kLayoutRunDual only): the words came from the copy with runs along y
template <int BPV, int LAYOUT, bool Q8>
__device__ __forceinline__ float tri_resolve(const TriFetch<BPV, LAYOUT> &f, const RayKernelArgs &a, float xb, float yb, float zb, bool along_y = false) {
	const float ax = filter_weight<Q8>(__builtin_amdgcn_fractf(__builtin_amdgcn_fmed3f(xb, 0.0f, a.max_x)));
	const float ay = filter_weight<Q8>(__builtin_amdgcn_fractf(__builtin_amdgcn_fmed3f(yb, 0.0f, a.max_y)));
	const float az = filter_weight<Q8>(__builtin_amdgcn_fractf(__builtin_amdgcn_fmed3f(zb, 0.0f, a.max_z)));
	float v000, v100, v010, v110, v001, v101, v011, v111;
	if (LAYOUT == kLayoutRunY) {                         // elements are (x,z) neighbourhoods, the two words are rows y and y+1
		v000 = (float) (f.w0 & 0xffu); v100 = (float) ((f.w0 >> 8) & 0xffu); v001 = (float) ((f.w0 >> 16) & 0xffu); v101 = (float) (f.w0 >> 24);
		v010 = (float) (f.w1 & 0xffu); v110 = (float) ((f.w1 >> 8) & 0xffu); v011 = (float) ((f.w1 >> 16) & 0xffu); v111 = (float) (f.w1 >> 24);
	} else if (LAYOUT == kLayoutRunDual) {               // either of the two: bytes 2, 3 of word 0 and bytes 0, 1 of word 1 change places
		const float t2 = (float) ((f.w0 >> 16) & 0xffu), t3 = (float) (f.w0 >> 24), t4 = (float) (f.w1 & 0xffu), t5 = (float) ((f.w1 >> 8) & 0xffu);
		v000 = (float) (f.w0 & 0xffu); v100 = (float) ((f.w0 >> 8) & 0xffu); v011 = (float) ((f.w1 >> 16) & 0xffu); v111 = (float) (f.w1 >> 24);
		v010 = along_y ? t4 : t2; v110 = along_y ? t5 : t3; v001 = along_y ? t2 : t4; v101 = along_y ? t3 : t5;
	} else if (LAYOUT != kLayoutLinear) {
		if (BPV == 1) {                                  // v_cvt_f32_ubyte0..3
			v000 = (float) (f.w0 & 0xffu); v100 = (float) ((f.w0 >> 8) & 0xffu); v010 = (float) ((f.w0 >> 16) & 0xffu); v110 = (float) (f.w0 >> 24);
			v001 = (float) (f.w1 & 0xffu); v101 = (float) ((f.w1 >> 8) & 0xffu); v011 = (float) ((f.w1 >> 16) & 0xffu); v111 = (float) (f.w1 >> 24);
		} else {
			v000 = (float) (f.w0 & 0xffffu); v100 = (float) (f.w0 >> 16); v010 = (float) (f.w1 & 0xffffu); v110 = (float) (f.w1 >> 16);
			v001 = (float) (f.w2 & 0xffffu); v101 = (float) (f.w2 >> 16); v011 = (float) (f.w3 & 0xffffu); v111 = (float) (f.w3 >> 16);
		}
	} else {
		if (BPV == 1) {
			v000 = (float) (f.w0 & 0xffu); v100 = (float) (f.w0 >> 8); v010 = (float) (f.w1 & 0xffu); v110 = (float) (f.w1 >> 8);
			v001 = (float) (f.w2 & 0xffu); v101 = (float) (f.w2 >> 8); v011 = (float) (f.w3 & 0xffu); v111 = (float) (f.w3 >> 8);
		} else {
			v000 = (float) (f.w0 & 0xffffu); v100 = (float) (f.w0 >> 16); v010 = (float) (f.w1 & 0xffffu); v110 = (float) (f.w1 >> 16);
			v001 = (float) (f.w2 & 0xffffu); v101 = (float) (f.w2 >> 16); v011 = (float) (f.w3 & 0xffffu); v111 = (float) (f.w3 >> 16);
		}
	}
	const float c00 = lerp(v000, v100, ax), c10 = lerp(v010, v110, ax);
	const float c01 = lerp(v001, v101, ax), c11 = lerp(v011, v111, ax);
	const float c0 = lerp(c00, c10, ay), c1 = lerp(c01, c11, ay);
	return lerp(c0, c1, az);
}

// x where the wave mask has the lane's bit set, 0 elsewhere: one v_cndmask with the mask taken straight from SGPRs
__device__ __forceinline__ float select_lanes(uint64_t mask, float x) {
	float r;
	asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(x), "s"(mask));
	return r;
}
// x where the wave mask has the lane's bit set, `other` elsewhere
__device__ __forceinline__ float select_lanes_else(uint64_t mask, float x, float other) {
	float r;
	asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(other), "v"(x), "s"(mask));
	return r;
}
enum : int { kFcmpOGT = 2, kFcmpOGE = 3, kFcmpOLE = 5, kFcmpUNE = 14, kIcmpNE = 33, kIcmpSGT = 38 };   // LLVM fcmp / icmp predicate codes for __builtin_amdgcn_fcmpf / sicmp

// Exact saturation shortcut, decided per wave.  A sample is composited with weight t = 1 - acc.w (CPURenderer.cpp:34); once a
// ray's accumulated alpha is EXACTLY 1.0f that weight is exactly 0 and every later sample leaves all four channels bit for
// bit unchanged (acc + c * 0 == acc, fma(c, 0, acc) == acc for finite c), whatever the early-termination threshold — with the
// reference's "no optims" threshold of 1.0 its own test `acc.w > threshold` never fires.  When no live lane of the wave has
// acc.w != 1.0 the wave therefore skips interpolation, transfer function, shading and compositing of the sample; the march
// itself (k, the fetches, the exit test) goes on unchanged.  Lanes the mask calls open: live and acc.w != 1 (NaN counts as open).
#ifdef VR_NO_SAT_SHORTCUT
#define VR_OPEN_LANES(acc_w, live) (live)
#else
#define VR_OPEN_LANES(acc_w, live) (__builtin_amdgcn_fcmpf((acc_w), 1.0f, kFcmpUNE) & (live))
#endif

// 1/sqrt(x) of the light vector in TRILINEAR mode: integer seed + three Newton steps in plain IEEE fp32 operations,
// identical on CPU and GPU (oracle/vr_oracle.c rsqrt_nr); relative error < 2e-7.
__device__ __forceinline__ float rsqrt_nr(float x) {
	float y = __uint_as_float(0x5f3759dfu - (__float_as_uint(x) >> 1));
	const float h = 0.5f * x;
	y = y * VR_FMA(-(h * y), y, 1.5f);
	y = y * VR_FMA(-(h * y), y, 1.5f);
	y = y * VR_FMA(-(h * y), y, 1.5f);
	return y;
}

// ---- per-ray helpers (reference order of operations) ------------------------------------------------------------

// RaycasterBase.h:32-42 Raycaster::intersect; min_bound = (-1,-1,-1) (ModelBase.cpp:10-14)
__device__ __forceinline__ bool intersect(f3 pt, f3 dir, float &kx, float &ky) {
	if (dir.x == 0) dir.x = 0.00001f;
	if (dir.y == 0) dir.y = 0.00001f;
	if (dir.z == 0) dir.z = 0.00001f;
	const float mb = -1.0f, nb = 1.0f;
	f3 k1 = mk3((mb - pt.x) / dir.x, (mb - pt.y) / dir.y, (mb - pt.z) / dir.z);
	f3 k2 = mk3((nb - pt.x) / dir.x, (nb - pt.y) / dir.y, (nb - pt.z) / dir.z);
	kx = flmax(flmax(flmin(k1.x, k2.x), flmin(k1.y, k2.y)), flmin(k1.z, k2.z));
	ky = flmin(flmin(flmax(k1.x, k2.x), flmax(k1.y, k2.y)), flmax(k1.z, k2.z));
	kx = flmax(kx, 0);
	return (kx < ky) && (ky > 0);
}

// n / esl_block_dims for n < 65536 without an integer divide: shift when the block edge is a power of two, otherwise the
// high half of n * (floor(2^32 / d) + 1), which is exact for n * d < 2^32 (host: RayKernelArgs::esl_div_*).
__device__ __forceinline__ uint32_t block_of(const RayKernelArgs &a, uint32_t n) {
	return a.esl_div_magic ? __umulhi(n, a.esl_div_magic) : (n >> a.esl_div_shift);
}

struct BlockIdx { uint32_t x, y, z; };
// block coordinates of a position: map_float_int((p + 1) / 2, dim) / esl_block_dims per axis (RaycasterBase.h:59-63,69-73)
__device__ __forceinline__ BlockIdx block_index(const RayKernelArgs &a, f3 pos) {
	BlockIdx b;
	b.x = block_of(a, map_float_int((pos.x + 1) * 0.5f, a.dim_x));
	b.y = block_of(a, map_float_int((pos.y + 1) * 0.5f, a.dim_y));
	b.z = block_of(a, map_float_int((pos.z + 1) * 0.5f, a.dim_z));
	return b;
}

// RaycasterBase.h:52-65 Raycaster::sample_data_esl — bit set = block is empty; table read from LDS (Tables: a unit's struct with the ESL words)
template <class Tables>
__device__ __forceinline__ bool block_empty(const Tables &t, BlockIdx b) {
	const uint32_t index = (b.z * VR_ESL_VOLUME_DIMS + b.y) & 0xffffu;          // `unsigned short index` in the reference
	const uint32_t word = t.esl[index & (VR_ESL_VOLUME_SIZE - 1)];
	return (word & (1u << (b.x & 31u))) != 0;
}

// RaycasterBase.h:67-85 Raycaster::leap_empty_space
__device__ __forceinline__ float leap_empty_space(const RayKernelArgs &a, BlockIdx b, f3 pt, f3 dir) {
	uint32_t ix = b.x, iy = b.y, iz = b.z;
	if (dir.x > 0) ix++;
	if (dir.y > 0) iy++;
	if (dir.z > 0) iz++;
	const f3 num = mk3((-1.0f + a.p.esl_block_size[0] * (float) ix) - pt.x, (-1.0f + a.p.esl_block_size[1] * (float) iy) - pt.y,
	                   (-1.0f + a.p.esl_block_size[2] * (float) iz) - pt.z);
	// Exact shortcut: a quotient num / dir is <= 0 when num is 0 (and dir is not) or when the signs differ, and one
	// non-positive quotient makes dk = max(min(..), 0) = 0, i.e. a leap of floor(0 / step) * step = 0 — no division needed.
	// That is the steady state of a ray that runs exactly along a block face (axis-aligned views): it probes every step.
	// The sign test is the product num * dir < 0 (a product that underflows to 0 just takes the division path), kept in
	// VGPR arithmetic: per-axis lane masks would cost SGPRs, and above 80 of them a SIMD holds 7 waves instead of 8.
	{
		const float sx = num.x == 0 ? -__builtin_fabsf(dir.x) : num.x * dir.x;
		const float sy = num.y == 0 ? -__builtin_fabsf(dir.y) : num.y * dir.y;
		const float sz = num.z == 0 ? -__builtin_fabsf(dir.z) : num.z * dir.z;
		if (__builtin_fminf(__builtin_fminf(sx, sy), sz) < 0)
			return 0.0f;
	}
	f3 kp = mk3(num.x / dir.x, num.y / dir.y, num.z / dir.z);
	if (dir.x == 0) kp.x = 100;
	if (dir.y == 0) kp.y = 100;
	if (dir.z == 0) kp.z = 100;
	float dk = flmin(kp.x, kp.y);
	dk = flmin(dk, kp.z);
	dk = flmax(dk, 0);
	return __builtin_floorf(dk / a.p.ray_step) * a.p.ray_step;
}

template <int SAMPLING>
__device__ __forceinline__ f3 march_point(f3 origin, f3 dir, float k) {
	if (SAMPLING == VR_SAMPLE_NEAREST)       // CPURenderer.cpp:17,24,38: origin + (direction * k), two roundings
		return mk3(origin.x + dir.x * k, origin.y + dir.y * k, origin.z + dir.z * k);
	return mk3(VR_FMA(dir.x, k, origin.x), VR_FMA(dir.y, k, origin.y), VR_FMA(dir.z, k, origin.z));
}

template <int I, int N, typename F> __device__ __forceinline__ void static_for(F &&body) {
	if constexpr (I < N) { body(std::integral_constant<int, I>()); static_for<I + 1, N>(body); }
}
// keeps a value in its register across this point (an inline-asm operand must not be a lambda capture, hence the functions)
__device__ __forceinline__ void pin(uint32_t &x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void pin(uint32_t &x, uint32_t &y) { asm volatile("" : "+v"(x), "+v"(y)); }
__device__ __forceinline__ void pin(uint32_t &x, uint32_t &y, uint32_t &z, uint32_t &w) { asm volatile("" : "+v"(x), "+v"(y), "+v"(z), "+v"(w)); }
__device__ __forceinline__ void pin(uint64_t &x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void pin(uint64_t &x, uint64_t &y) { asm volatile("" : "+v"(x), "+v"(y)); }
__device__ __forceinline__ void pin(u32x4 &x) { asm volatile("" : "+v"(x)); }
template <int I> __device__ __forceinline__ void managed_wait() {       // s_waitcnt vmcnt(I): all but the I youngest gathers have landed
	static_assert(I >= 0 && I <= 63, "vmcnt is a 6-bit field on gfx9");
	asm volatile("s_waitcnt vmcnt(%0)" : : "n"(I));
}

// -- workgroup -> tile map, chosen by measurement on the 8-XCD chip (scripts/gpu_variants.sh, lit full march, 8-view
//    mean).  Tiles are numbered in BxB-tile blocks (B = 8: 256x128 pixels), so the ~1000 workgroups in flight at any time
//    cover a compact screen region and share bricks in both screen directions (row-major numbering: +3..7 %).  Workgroups
//    are dealt round-robin over the XCDs (b and b + 8 share an L2); three assignments of tiles to XCDs were measured:
//      0  tile = workgroup id — every block is spread over all eight XCDs (XCD x renders column x of each block)   4.66 ms
//      1  each XCD owns one contiguous eighth of the tile list (one screen band per L2)                            6.25 ms
//      2  each XCD owns whole blocks, interleaved over the frame                                                   6.06 ms
//    Concentrating a compact brick region on ONE L2 (1, 2) is markedly slower than letting all eight L2s serve it —
//    the reuse between neighbouring tiles is small (the quad elements already carry the +1 neighbours) and a compact
//    region exercises few L2 channels.  Round 4 (C4 full march, 8 views): WHICH tiles of a block share an XCD matters a little —
//      3  pairs of x-neighbours   2.43 ms (views 1 / 4 / 5)      4  2x2 quads   2.42      0  columns   2.43
//      5  XCD x renders ROW x of each block: 2.38 on those views, 2.069 against 2.093 over all eight (x-neighbours read
//         neighbouring bricks of the x-fastest brick order); frames that launch in a measured-cost order: 0.599 against 0.594.
//    Placement affects speed only.  5 is the numbering of the tiles inside a block (column-major), the same for every frame, and
//    the host's tile_number_to_xy (vr_device.h, where VR_XCD_MODE is defined) follows it.
#ifndef VR_COL_XCD_MODE
#define VR_COL_XCD_MODE 0              // the column kernels' own choice
#endif
constexpr uint32_t kTileBlock = VR_TILE_ORDER > 1 ? VR_TILE_ORDER : 1;
// tile number (the launch-order entry, or the workgroup id `bid`) -> workgroup tile column / row
template <int XCD_MODE = VR_XCD_MODE>
__device__ __forceinline__ void tile_to_xy(uint32_t tiles_x, uint32_t tiles_y, uint32_t tile, uint32_t bid, uint32_t &tile_x, uint32_t &tile_y) {
	constexpr uint32_t B = kTileBlock;
	const uint32_t ntiles = tiles_x * tiles_y;
	const uint32_t full_cols = tiles_x / B, full_rows = tiles_y / B;
	const uint32_t nblocked = full_cols * full_rows * B * B;          // tiles that lie in complete BxB blocks
	if (XCD_MODE == 1) {                                           // contiguous chunk of the tile list per XCD
		const uint32_t xcd = bid & 7u, slot = bid >> 3, q = ntiles >> 3, r = ntiles & 7u;
		tile = xcd * q + (xcd < r ? xcd : r) + slot;
	} else if (XCD_MODE == 2) {                                    // whole blocks per XCD, interleaved over the frame
		const uint32_t covered = (nblocked / (8u * B * B)) * (8u * B * B);
		if (bid < covered) {
			const uint32_t set = bid / (8u * B * B), within = bid - set * (8u * B * B);
			tile = (set * 8u + (within & 7u)) * (B * B) + (within >> 3);
		}
	}
	tile_y = tile / tiles_x; tile_x = tile - tile_y * tiles_x;
	if (B > 1) {
		if (tile < nblocked) {
			const uint32_t blk = tile / (B * B), in = tile - blk * (B * B);
			uint32_t by = blk / full_cols, bx = blk - by * full_cols;
#ifdef VR_CENTER_FIRST
			// blocks from the middle of the frame outwards: the long / opaque rays of a centred object start first
			by = (by & 1u) ? full_rows / 2u - 1u - (by >> 1) : full_rows / 2u + (by >> 1);
			bx = (bx & 1u) ? full_cols / 2u - 1u - (bx >> 1) : full_cols / 2u + (bx >> 1);
#endif
			uint32_t ix = in % B, iy = in / B;
			if (B == 8 && XCD_MODE >= 3) {                // which tiles of a block share an XCD (= in & 7 in workgroup order): 3 pairs along x, 4 2x2 quads, 5 rows
				const uint32_t xcd = in & 7u, slot = in >> 3;
				if (XCD_MODE == 3) { ix = ((xcd & 3u) << 1) | (slot & 1u); iy = ((slot >> 1) << 1) | (xcd >> 2); }
				else if (XCD_MODE == 4) { ix = ((xcd & 3u) << 1) | (slot & 1u); iy = ((slot >> 1) & 1u) | ((xcd >> 2) << 1) | ((slot >> 2) << 2); }
				else { ix = slot; iy = xcd; }
			}
			tile_x = bx * B + ix; tile_y = by * B + iy;
		} else {                                      // ragged right / bottom margins: leftover tiles, row-major
			uint32_t rest = tile - nblocked;
			const uint32_t right_w = tiles_x - full_cols * B, right_n = right_w * full_rows * B;
			if (rest < right_n) { tile_y = rest / right_w; tile_x = full_cols * B + rest % right_w; }
			else { rest -= right_n; tile_y = full_rows * B + rest / tiles_x; tile_x = rest % tiles_x; }
		}
	}

}

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t) __builtin_amdgcn_readfirstlane((int) v); }
__device__ __forceinline__ float rlane(float v, int lane) { return __uint_as_float((uint32_t) __builtin_amdgcn_readlane((int) __float_as_uint(v), lane)); }
// the values must be in scalar registers HERE: scalar loads that produce them are issued together before this point and waited for once
template <typename T> __device__ __forceinline__ void hold_scalar(const T &v) { asm volatile("" :: "s"(v)); }
template <typename... T> __device__ __forceinline__ void hold_scalars(const T &...v) { (void) std::initializer_list<int>{ (hold_scalar(v), 0)... }; }

// -- lane -> pixel of the frame buffer, for a workgroup of THREADS threads on tile (tile_x, tile_y): lx / ly wrap for the pixels left of /
//    below the buffer (tile phase).  One wavefront = one 8x8 pixel tile; 8 waves = 32x16 pixels, 16 waves = 32x32.  Inside the wave each
//    group of 16 consecutive lanes is a 4x4-pixel block (not two 8-pixel rows): a compact block keeps the group's samples inside the
//    fewest cache sectors whatever the view direction.  SQUARE_WAVES: the wave shape is 8x8 whatever lane_map says (the column kernels).
template <uint32_t THREADS, bool SQUARE_WAVES = false>
__device__ __forceinline__ void lane_pixel(const RayKernelArgs &a, uint32_t tile_x, uint32_t tile_y, uint32_t &lx, uint32_t &ly) {
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t qd = lane >> 4;
	// Order of the 16 lanes inside the group, picked per frame by the host (vr_hip_api.cpp choose_tile_mapping): the vector
	// memory pipeline handles 4 consecutive lanes together and is fastest when their addresses share one aligned 16-byte
	// chunk, so the 4 lanes should be the 4 pixels whose samples lie closest together in the brick order.
	uint32_t gu = lane & 3u, gv = (lane >> 2) & 3u;                             // kLaneRows: lanes run along screen x
	const uint32_t order = a.lane_map & 3u, shape = THREADS == 512u && !SQUARE_WAVES ? (a.lane_map >> 2) : 0u;
	if (order == kLaneBlocks) { gu = ((lane >> 1) & 2u) | (lane & 1u); gv = ((lane >> 2) & 2u) | ((lane >> 1) & 1u); }
	else if (order == kLaneColumns) { const uint32_t t = gu; gu = gv; gv = t; }
	// Shape of the wave's pixel tile inside the 32x16-pixel workgroup tile (bits 2.. of lane_map): 0 = 8x8 (four 4x4 groups as 2x2),
	// 1 = 16 wide x 4 high (the groups side by side; the 8 waves 2 across x 4 down), 2 = 4 wide x 16 high (8 waves across).
	uint32_t wx, wy, ox, oy;
	if (shape == 1u) { wx = qd * 4u + gu; wy = gv; ox = (wave & 1u) * 16u; oy = (wave >> 1) * 4u; }
	else if (shape == 2u) { wx = gu; wy = qd * 4u + gv; ox = wave * 4u; oy = 0u; }
	else { wx = (qd & 1u) * 4u + gu; wy = (qd >> 1) * 4u + gv; ox = (wave & 3u) * 8u; oy = (wave >> 2) * 8u; }
	lx = tile_x * 32u + ox + wx - a.phase_x;
	ly = tile_y * (THREADS / 32u) + oy + wy - a.phase_y;
}
// row of the frame buffer -> row of the view (the band partition of vr_render_params)
__device__ __forceinline__ uint32_t frame_row(const RayKernelArgs &a, uint32_t ly) {
	const uint32_t band = ly / a.p.band_rows;
	return (band * a.p.band_stride + a.p.band_first) * a.p.band_rows + (ly - band * a.p.band_rows);
}

// -- the ray of view pixel (gx, gy): View::get_ray (ViewBase.h:23-35, its order of operations), Raycaster::intersect and the
//    termination guard, once per ray instead of a counter per sample: k advances by `step` every iteration as long as
//    ky + step != ky (fp32 spacing grows with magnitude, so that holds for every k <= ky), and the march is cut after
//    kMaxRaySteps steps.  Neither condition can trigger for a view the reference can produce (k spans <= 2*sqrt(3)).
//    Returned by value, the view read by index: handed out through references (or read through ld3) the ray lands in scratch.
//    ORTHOGONAL: for kernels the host never launches for a perspective view — their direction stays the wave-uniform kernel argument.
struct PixelRay { f3 origin, dir; float kx, ky; bool alive; };
template <bool ORTHOGONAL = false>
__device__ __forceinline__ PixelRay pixel_ray(const RayKernelArgs &a, uint32_t gx, uint32_t gy) {
	PixelRay r;
	const float fx = (float) ((int) gx - (int) (a.p.view.width / 2u));
	const float fy = (float) ((int) gy - (int) (a.p.view.height / 2u));
	const f3 vo = mk3(a.p.view.origin[0], a.p.view.origin[1], a.p.view.origin[2]);
	const f3 vd = mk3(a.p.view.direction[0], a.p.view.direction[1], a.p.view.direction[2]);
	const f3 vr_ = mk3(a.p.view.right_plane[0], a.p.view.right_plane[1], a.p.view.right_plane[2]);
	const f3 vu = mk3(a.p.view.up_plane[0], a.p.view.up_plane[1], a.p.view.up_plane[2]);
	if (!ORTHOGONAL && a.p.view.perspective) {
		r.origin = vo;
		r.dir = mk3(vd.x + vr_.x * fx, vd.y + vr_.y * fx, vd.z + vr_.z * fx);
		r.dir = mk3(r.dir.x + vu.x * fy, r.dir.y + vu.y * fy, r.dir.z + vu.z * fy);
	} else {
		r.dir = vd;
		r.origin = mk3(vo.x + vr_.x * fx, vo.y + vr_.y * fx, vo.z + vr_.z * fx);
		r.origin = mk3(r.origin.x + vu.x * fy, r.origin.y + vu.y * fy, r.origin.z + vu.z * fy);
	}
	r.kx = 0; r.ky = 0;
	r.alive = gx < a.p.view.width && gy < a.p.view.height;
	r.alive = r.alive && intersect(r.origin, r.dir, r.kx, r.ky);
	const float step = a.p.ray_step;
	r.alive = r.alive && (r.ky + step > r.ky);
	r.ky = flmin(r.ky, r.kx + step * (float) kMaxRaySteps);
	return r;
}

// -- the clip region of a clipped frame (include/vr_hip.h vr_hip_set_clip), applied to the segment pixel_ray found:
//    the crop box narrows [kx, ky] by intersect's own slab arithmetic (exact zeros of the direction replaced, IEEE divisions, its order of
//    flmin / flmax — the box [-1,1]^3 changes no bit), the plane by the parameter at which the ray crosses it, formed from the unreplaced
//    direction.  Returns intersect's hit test on the narrowed segment; a miss is a miss of the cube.  The two guards of pixel_ray have
//    looked at the unclipped segment, which contains this one.
//    The ten constants are read HERE, behind the table staging, through a laundered pointer to the kernel-argument segment (the dual_bits
//    pattern of vr_raymarch_body.inc; RayKernelArgs is the first argument of all three kernels: offset 0): read as members of the by-value argument
//    they are loaded at the kernel's entry with the rest of it and stay live across the staging code, the SGPR peak — measured +10 SGPRs on
//    every instantiation.
__device__ __forceinline__ bool clip_segment(f3 origin, f3 dir, float &kx, float &ky) {
	typedef const RayKernelArgs __attribute__((address_space(4))) *ConstArgs;      // constant address space: scalar loads
	ConstArgs a = (ConstArgs) __builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(a));
	f3 d = dir;
	if (d.x == 0) d.x = 0.00001f;
	if (d.y == 0) d.y = 0.00001f;
	if (d.z == 0) d.z = 0.00001f;
	const f3 k1 = mk3((a->clip_min[0] - origin.x) / d.x, (a->clip_min[1] - origin.y) / d.y, (a->clip_min[2] - origin.z) / d.z);
	const f3 k2 = mk3((a->clip_max[0] - origin.x) / d.x, (a->clip_max[1] - origin.y) / d.y, (a->clip_max[2] - origin.z) / d.z);
	const float kxb = flmax(flmax(flmin(k1.x, k2.x), flmin(k1.y, k2.y)), flmin(k1.z, k2.z));
	const float kyb = flmin(flmin(flmax(k1.x, k2.x), flmax(k1.y, k2.y)), flmax(k1.z, k2.z));
	kx = flmax(kx, kxb);
	ky = flmin(ky, kyb);
	const float dn = VR_FMA(a->clip_plane[2], dir.z, VR_FMA(a->clip_plane[1], dir.y, a->clip_plane[0] * dir.x));
	const float on = VR_FMA(a->clip_plane[2], origin.z, VR_FMA(a->clip_plane[1], origin.y, VR_FMA(a->clip_plane[0], origin.x, a->clip_plane[3])));
	bool kept = true;
	if (dn > 0) kx = flmax(kx, -on / dn);
	else if (dn < 0) ky = flmin(ky, -on / dn);
	else kept = on >= 0;                            // the ray runs inside the plane's direction (no plane: 0 >= 0)
	return kept && (kx < ky) && (ky > 0);
}

// -- empty space leaping (CPURenderer.cpp:18-25): the composite's loop in its plain per-lane form, on the ESL words of the unit's tables
//    (depth_kernel, label_kernel).  What else these kernels and section_kernel repeat — the pixel prologue, the reset of lanes without a sample
//    with A / B, the batch issue — stays written out in them: as functions each changed the machine code of some row (scripts/kernel_diff.py).
template <int SAMPLING, class Tables>
__device__ __forceinline__ void leap_lane(const RayKernelArgs &a, const Tables &t, f3 origin, f3 dir, float &kx, float ky, bool alive) {
	if (!a.p.esl) return;
	const float step = a.p.ray_step;
	f3 pt = march_point<SAMPLING>(origin, dir, kx);
	bool probing = alive;
	while (__builtin_amdgcn_ballot_w64(probing) != 0ull) {
		if (probing) {
			const BlockIdx blk = block_index(a, pt);
			if (kx <= ky && block_empty(t, blk)) {
				kx += leap_empty_space(a, blk, pt, dir);
				kx += step;
				pt = march_point<SAMPLING>(origin, dir, kx);
			} else {
				probing = false;
			}
		}
	}
}

// -- the factor of a shadowed composite frame (include/vr_hip.h vr_hip_set_shadow) for the sample at model-space point
//    pt: f = fma(strength / 255, Tq, 1 - strength), Tq the trilinear interpolation of the light grid's bytes q at pt — node coordinate
//    fmed3(fma(pt, hs, hs), 0, S - 1), cell min((uint32_t) v, S - 2), weight v - cell, lerps along x, then y, then z, full fp32 weights in
//    both sampling modes.  The cell index is at most S - 2 whatever pt is (a NaN converts to 0), so the eight byte loads stay inside the S^3
//    bytes for every lane, live or not.  The constants come through the laundered kernel-argument pointer, as in clip_segment: only the few
//    samples that are dense get here, and nothing of the grid occupies a scalar register across the march.
__device__ __forceinline__ float shadow_factor(f3 pt) {
	typedef const RayKernelArgs __attribute__((address_space(4))) *ConstArgs;
	ConstArgs a = (ConstArgs) __builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(a));
	const float hs = a->shadow_hs, top = a->shadow_max;
	const uint32_t last = a->shadow_last, row = a->shadow_row, slab = a->shadow_slab;
	float vx = __builtin_amdgcn_fmed3f(VR_FMA(pt.x, hs, hs), 0.0f, top);
	float vy = __builtin_amdgcn_fmed3f(VR_FMA(pt.y, hs, hs), 0.0f, top);
	float vz = __builtin_amdgcn_fmed3f(VR_FMA(pt.z, hs, hs), 0.0f, top);
	auto cell = [&](float v) { const uint32_t i = (uint32_t) v; return i < last ? i : last; };
	// Register diet (the dense block sits inside the march's prefetch pipeline, whose fetch slots stay live): the three node coordinates and
	// one offset cross the loads, the cells and weights are formed again from the coordinates behind them, one slab's four bytes at a time
	uint32_t off = (cell(vz) * slab + cell(vy) * row) + cell(vx);
	asm volatile("" : "+v"(off), "+v"(vx), "+v"(vy), "+v"(vz));
	const uint8_t *q = (const uint8_t *) (uintptr_t) a->shadow_q + off;
	uint32_t b0 = q[0], b1 = q[1], b2 = q[row], b3 = q[row + 1u];
	asm volatile("" : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3));
	const float wx = vx - (float) cell(vx);
	float c00 = lerp((float) b0, (float) b1, wx), c10 = lerp((float) b2, (float) b3, wx);
	asm volatile("" : "+v"(c00), "+v"(c10));
	const uint8_t *q1 = q + slab;
	uint32_t b4 = q1[0], b5 = q1[1], b6 = q1[row], b7 = q1[row + 1u];
	asm volatile("" : "+v"(b4), "+v"(b5), "+v"(b6), "+v"(b7));
	const float c01 = lerp((float) b4, (float) b5, wx), c11 = lerp((float) b6, (float) b7, wx);
	const float wy = vy - (float) cell(vy), wz = vz - (float) cell(vz);
	const float tq = lerp(lerp(c00, c10, wy), lerp(c01, c11, wy), wz);
	return VR_FMA(a->shadow_scale, tq, a->shadow_base);
}

// -- the Blinn-Phong term of a gradient-lit composite frame (include/vr_hip.h vr_hip_set_lighting steps 1-4) for the
//    sample k of the ray (origin, dir) — texel coordinates fma(k, A, B), model-space point march_point(origin, dir, k); `lit` = the wave mask
//    of the lanes whose looked-up colour is dense.  The gradient is the isosurface's (vr_iso_body.inc): central differences one texel apart of
//    the interpolated raw value with clamp addressing, so all six fetches are in bounds for every lane, live or not.  Register diet (the dense
//    block sits inside the march's prefetch pipeline, whose fetch slots stay live): one axis at a time — at most two fetches in flight,
//    the difference formed, then the next axis.  The constants and the light come through the laundered kernel-argument pointer, as in
//    clip_segment and shadow_factor: nothing of them occupies a scalar register across the march.  Returns m and spec of step 4 (1 and 0
//    for the lanes that are not lit): the caller forms c.xyz = fma(c.xyz, m, spec) and leaves c.w alone.
template <int BPV, int ADDR, int LAYOUT, bool Q8>
__device__ __forceinline__ void light_sample(const void *vol, const RayKernelArgs &ka, const uint32_t *lut, f3 A, f3 B, f3 origin, f3 dir, float kx,
                                             uint64_t lit, float cw, float &m_out, float &spec_out) {
	typedef const RayKernelArgs __attribute__((address_space(4))) *ConstArgs;
	ConstArgs a = (ConstArgs) __builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(a));
	// one axis: the two fetches issued, the texel coordinates formed again from k behind the loads (the same fused multiply-adds, the same
	// bits) instead of carried across them, the difference scaled; the scheduling barrier keeps the next axis' loads behind this one's use.
	// Both fetches of an axis are in flight where the registers allow it — 1-byte voxels in quad bricks behind address tables, the default
	// path —, one after the other elsewhere (four-word fetches, 64-bit addresses: DESIGN.md section 4.8 has the figures of both forms)
	constexpr bool kPair = BPV == 1 && LAYOUT == kLayoutBricked && ADDR != kAddrWide;
	auto central = [&](auto axis) -> float {
		constexpr int X = decltype(axis)::value;
		float k = kx;
		asm volatile("" : "+v"(k));
		float xb = VR_FMA(k, A.x, B.x), yb = VR_FMA(k, A.y, B.y), zb = VR_FMA(k, A.z, B.z);
		const TriFetch<BPV, LAYOUT> fp = tri_issue<BPV, ADDR, LAYOUT>(vol, ka, lut, X == 0 ? xb + 1.0f : xb, X == 1 ? yb + 1.0f : yb, X == 2 ? zb + 1.0f : zb, true);
		TriFetch<BPV, LAYOUT> fm;
		if constexpr (kPair) fm = tri_issue<BPV, ADDR, LAYOUT>(vol, ka, lut, X == 0 ? xb - 1.0f : xb, X == 1 ? yb - 1.0f : yb, X == 2 ? zb - 1.0f : zb, true);
		__builtin_amdgcn_sched_barrier(0);
		asm volatile("" : "+v"(k));
		xb = VR_FMA(k, A.x, B.x); yb = VR_FMA(k, A.y, B.y); zb = VR_FMA(k, A.z, B.z);
		float vp = tri_resolve<BPV, LAYOUT, Q8>(fp, ka, X == 0 ? xb + 1.0f : xb, X == 1 ? yb + 1.0f : yb, X == 2 ? zb + 1.0f : zb);
		if constexpr (!kPair) {
			asm volatile("" : "+v"(vp), "+v"(k));
			__builtin_amdgcn_sched_barrier(0);
			xb = VR_FMA(k, A.x, B.x); yb = VR_FMA(k, A.y, B.y); zb = VR_FMA(k, A.z, B.z);
			fm = tri_issue<BPV, ADDR, LAYOUT>(vol, ka, lut, X == 0 ? xb - 1.0f : xb, X == 1 ? yb - 1.0f : yb, X == 2 ? zb - 1.0f : zb, true);
			__builtin_amdgcn_sched_barrier(0);
			asm volatile("" : "+v"(k));
			xb = VR_FMA(k, A.x, B.x); yb = VR_FMA(k, A.y, B.y); zb = VR_FMA(k, A.z, B.z);
		}
		const float vm = tri_resolve<BPV, LAYOUT, Q8>(fm, ka, X == 0 ? xb - 1.0f : xb, X == 1 ? yb - 1.0f : yb, X == 2 ? zb - 1.0f : zb);
		float g = (vp - vm) * (X == 0 ? a->half_x : (X == 1 ? a->half_y : a->half_z));
		asm volatile("" : "+v"(g));
		__builtin_amdgcn_sched_barrier(0);
		return g;
	};
	const float gx = central(std::integral_constant<int, 0>()), gy = central(std::integral_constant<int, 1>()), gz = central(std::integral_constant<int, 2>());
	const f3 pt = march_point<VR_SAMPLE_TRILINEAR>(origin, dir, kx);
	const float gg = VR_FMA(gz, gz, VR_FMA(gy, gy, gx * gx));
	lit &= __builtin_amdgcn_fcmpf(gg, 0.0f, kFcmpOGT);                          // a plateau has no surface to light: the sample stays as looked up
	m_out = 1.0f; spec_out = 0.0f;
	if (lit == 0ull) return;
	const float ig = rsqrt_nr(gg);
	const f3 dl = mk3(a->p.view.light_pos[0] - pt.x, a->p.view.light_pos[1] - pt.y, a->p.view.light_pos[2] - pt.z);
	const float ll = VR_FMA(dl.z, dl.z, VR_FMA(dl.y, dl.y, dl.x * dl.x));
	const float il = rsqrt_nr(ll);
	const float dot = VR_FMA(gz, dl.z, VR_FMA(gy, dl.y, gx * dl.x));
	const float sd = ll > 0.0f ? __builtin_fminf(__builtin_fabsf((dot * ig) * il), 1.0f) : 0.0f;      // two-sided, as the isosurface is
	const float iv = rsqrt_nr(VR_FMA(dir.z, dir.z, VR_FMA(dir.y, dir.y, dir.x * dir.x)));
	const f3 h = mk3(VR_FMA(-dir.x, iv, dl.x * il), VR_FMA(-dir.y, iv, dl.y * il), VR_FMA(-dir.z, iv, dl.z * il));
	const float hh = VR_FMA(h.z, h.z, VR_FMA(h.y, h.y, h.x * h.x));
	float sp = __builtin_fminf(__builtin_fabsf((VR_FMA(gz, h.z, VR_FMA(gy, h.y, gx * h.x)) * ig) * rsqrt_nr(hh)), 1.0f);
	sp = (ll > 0.0f && hh > 0.0f) ? sp : 0.0f;
	for (uint32_t n = a->light_n; n != 0u; n--) sp = sp * sp;                   // the power 2^n by n squarings: no powf, CPU and GPU share every bit
	m_out = select_lanes_else(lit, VR_FMA(a->light_kd, sd, a->light_ka), 1.0f);    // fma(c, 1, 0) == c: other lanes unchanged
	spec_out = select_lanes(lit, (a->light_ks * sp) * cw);                      // the highlight is white and premultiplied
}
// whether the gradient-lit frame is shadowed too (wave-uniform; read where it is used, like the constants above)
__device__ __forceinline__ bool lit_frame_shadowed() {
	typedef const RayKernelArgs __attribute__((address_space(4))) *ConstArgs;
	ConstArgs a = (ConstArgs) __builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(a));
	return a->shadow_on != 0u;
}

// -- the opaque layer of a backdrop frame (include/vr_hip.h vr_backdrop), for the composite_backdrop* kernels alone: the
//    depth and the colour word of element `px` (= ly * out_width + lx, the layout of the output buffer).  The two addresses come through the
//    laundered kernel-argument pointer, as in clip_segment, so nothing of the layer occupies a scalar register across the march; they are
//    addresses, not __restrict__ pointers, and the output pointer of those kernels carries no __restrict__ either: the output may be the
//    colour layer.  A pixel reads its own elements before it stores its own output element, so in-place frames are well defined.
__device__ __forceinline__ float backdrop_depth_at(size_t px) {
	typedef const RayKernelArgs __attribute__((address_space(4))) *ConstArgs;
	ConstArgs a = (ConstArgs) __builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(a));
	return ((const float *) (uintptr_t) a->backdrop_depth)[px];
}
__device__ __forceinline__ uint32_t backdrop_rgba_at(size_t px) {
	typedef const RayKernelArgs __attribute__((address_space(4))) *ConstArgs;
	ConstArgs a = (ConstArgs) __builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(a));
	return ((const uint32_t *) (uintptr_t) a->backdrop_rgba)[px];
}
// ... and the output address of element px: the kernels' arguments are (RayKernelArgs, vol, tf, esl, out, ...), so the output pointer lies
// three pointers behind the first argument in the kernel-argument segment — read again there, behind the march, instead of kept across it
struct RayKernelSegment { RayKernelArgs a; const void *vol; const float *tf; const uint32_t *esl; uint32_t *out; };
__device__ __forceinline__ uint32_t *backdrop_out_at(size_t px) {
	typedef const RayKernelSegment __attribute__((address_space(4))) *ConstSegment;
	ConstSegment s = (ConstSegment) __builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(s));
	return s->out + px;
}

// -- the address tables of the quad / voxel / oct bricks into LDS; no barrier.  Entry j of a table belongs to cell
//    clamp(j - kLutPad, 0, dim - 1): the pad entries repeat the edge cells.
__device__ __forceinline__ uint32_t lut_cell_of(uint32_t j, uint32_t n) { const int c = (int) j - kLutPad; return (uint32_t) (c < 0 ? 0 : (c > (int) n - 1 ? (int) n - 1 : c)); }
template <int BPV, int ADDR, int LAYOUT>
__device__ __forceinline__ void stage_brick_tables(const RayKernelArgs &a, uint32_t *lut) {
	typedef LutCfg<ADDR> L;
	constexpr uint32_t kThreads = L::threads;
	const uint32_t t = threadIdx.x;
	const uint32_t nx = a.dim_x, ny = a.dim_y, nz = a.dim_z;
	const uint32_t elem = LAYOUT == kLayoutVoxel ? BPV : (LAYOUT == kLayoutOct ? 8u * BPV : 4u * BPV);   // bytes per element: one voxel, a quad, or the 2x2x2 neighbourhood
#ifdef VR_BOUNDS_CHECK
	if (t == 0) { bc_table_entries[0] = nx + 2 * kLutPad; bc_table_entries[1] = ny + 2 * kLutPad; bc_table_entries[2] = nz + 2 * kLutPad; }
#endif
	const uint32_t row = a.nbx * kBrickPitch;                        // elements per brick row / slab
	const uint64_t slab = (uint64_t) a.nby * row;
	for (uint32_t jj = t; jj < nz + 2 * kLutPad; jj += kThreads) {
		const uint32_t i = lut_cell_of(jj, nz);
		const uint32_t j = i + 1 < nz ? i + 1 : i;
		const uint64_t z0 = ((i >> 3) * slab + brick_spread(BPV, a.brick_plane, 2, i & 7u)) * elem;
		const uint64_t z1 = ((j >> 3) * slab + brick_spread(BPV, a.brick_plane, 2, j & 7u)) * elem;
		if (ADDR == kAddr32) {
			lut[2 * jj] = (uint32_t) z0; lut[2 * jj + 1] = (uint32_t) z1;
		} else {
			lut[4 * jj] = (uint32_t) z0; lut[4 * jj + 1] = (uint32_t) (z0 >> 32);
			lut[4 * jj + 2] = (uint32_t) z1; lut[4 * jj + 3] = (uint32_t) (z1 >> 32);
		}
	}
	for (uint32_t j = t; j < nx + 2 * kLutPad; j += kThreads) { const uint32_t i = lut_cell_of(j, nx); lut[L::x_at + j] = ((i >> 3) * kBrickPitch + brick_spread(BPV, a.brick_plane, 0, i & 7u)) * elem; }
	for (uint32_t j = t; j < ny + 2 * kLutPad; j += kThreads) { const uint32_t i = lut_cell_of(j, ny); lut[L::y_at + j] = ((i >> 3) * row + brick_spread(BPV, a.brick_plane, 1, i & 7u)) * elem; }
}

// Which instantiation a frame runs: ONE selector, visited by the launcher and by the host's questions about the launch (does it read
// the linear array?  how many workgroup tiles?), so the answers cannot drift from what is launched.  `visit` is called with four
// std::integral_constant tags <SAMPLING, BPV, ADDR, LAYOUT> and a bool: true = the variant reads `linear`, false = the brick copy.
template <int SAMPLING, int BPV, class F>
static auto select_sampling(const RayKernelArgs &a, bool have_bricked, F &&visit) {
	constexpr bool nearest = SAMPLING == VR_SAMPLE_NEAREST;
	typedef std::integral_constant<int, SAMPLING> S;
	typedef std::integral_constant<int, BPV> V;
	const uint32_t max_dim = a.dim_x > a.dim_y ? (a.dim_x > a.dim_z ? a.dim_x : a.dim_z) : (a.dim_y > a.dim_z ? a.dim_y : a.dim_z);
	if constexpr (!nearest && BPV == 1) {
		if (have_bricked && a.layout == kLayoutRun)
			return visit(S(), V(), std::integral_constant<int, kAddr32>(), std::integral_constant<int, kLayoutRun>(), false);
		if (have_bricked && a.layout == kLayoutRunY)
			return visit(S(), V(), std::integral_constant<int, kAddr32>(), std::integral_constant<int, kLayoutRunY>(), false);
		if (have_bricked && a.layout == kLayoutRunDual)
			return visit(S(), V(), std::integral_constant<int, kAddr32>(), std::integral_constant<int, kLayoutRunDual>(), false);
	}
	if constexpr (nearest) {
		if (have_bricked && a.layout == kLayoutVoxel) {
			if (max_dim <= LutCfg<kAddr32>::max_dim && a.force_wide != 2)
				return visit(S(), V(), std::integral_constant<int, kAddr32>(), std::integral_constant<int, kLayoutVoxel>(), false);
			return visit(S(), V(), std::integral_constant<int, kAddrLut64>(), std::integral_constant<int, kLayoutVoxel>(), false);
		}
	}
	if constexpr (!nearest && BPV == 2) {
		if (have_bricked && a.layout == kLayoutOct) {
			const uint64_t bytes = bricked_elems(a.dim_x, a.dim_y, a.dim_z) * 8 * BPV;
			if (!a.force_wide && max_dim <= LutCfg<kAddr32>::max_dim && bytes <= (1ull << 32))
				return visit(S(), V(), std::integral_constant<int, kAddr32>(), std::integral_constant<int, kLayoutOct>(), false);
			return visit(S(), V(), std::integral_constant<int, kAddrLut64>(), std::integral_constant<int, kLayoutOct>(), false);
		}
	}
	if (have_bricked && a.layout == kLayoutBricked) {
		const uint64_t bytes = bricked_elems(a.dim_x, a.dim_y, a.dim_z) * 4 * BPV;
		if (!a.force_wide && max_dim <= LutCfg<kAddr32>::max_dim && bytes <= (1ull << 32))
			return visit(S(), V(), std::integral_constant<int, kAddr32>(), std::integral_constant<int, kLayoutBricked>(), false);
		if (a.force_wide != 1 && max_dim <= LutCfg<kAddrLut64>::max_dim)
			return visit(S(), V(), std::integral_constant<int, kAddrLut64>(), std::integral_constant<int, kLayoutBricked>(), false);
		if constexpr (!nearest)
			return visit(S(), V(), std::integral_constant<int, kAddrWide>(), std::integral_constant<int, kLayoutBricked>(), false);
	}
	// the reference's linear array; 32-bit byte offsets cover every volume the reference can express (ModelBase.h:12)
	const bool wide = a.force_wide || ((uint64_t) a.dim_x * a.dim_y * a.dim_z + volume_tail_slack(a.dim_x, a.dim_y)) * BPV >= (1ull << 32);
	return wide ? visit(S(), V(), std::integral_constant<int, kAddrWide>(), std::integral_constant<int, kLayoutLinear>(), true)
	            : visit(S(), V(), std::integral_constant<int, kAddr32>(), std::integral_constant<int, kLayoutLinear>(), true);
}

template <class F>
static auto select_variant(const RayKernelArgs &a, bool have_bricked, uint32_t bpv, F &&visit) {
	if (bpv == 1) {
		if (a.p.sampling == VR_SAMPLE_NEAREST) return select_sampling<VR_SAMPLE_NEAREST, 1>(a, have_bricked, visit);
		if (a.p.sampling == VR_SAMPLE_TRILINEAR_Q8) return select_sampling<VR_SAMPLE_TRILINEAR_Q8, 1>(a, have_bricked, visit);
		return select_sampling<VR_SAMPLE_TRILINEAR, 1>(a, have_bricked, visit);
	}
	if (a.p.sampling == VR_SAMPLE_NEAREST) return select_sampling<VR_SAMPLE_NEAREST, 2>(a, have_bricked, visit);
	if (a.p.sampling == VR_SAMPLE_TRILINEAR_Q8) return select_sampling<VR_SAMPLE_TRILINEAR_Q8, 2>(a, have_bricked, visit);
	return select_sampling<VR_SAMPLE_TRILINEAR, 2>(a, have_bricked, visit);
}

// f(std::integral_constant<int, AXIS>, std::bool_constant<FLAG>) for a runtime axis (0, 1; anything else: 2) and flag: the kernels
// that are instantiated per march axis and one switch
template <class F>
static void dispatch_axis_flag(uint32_t axis, bool flag, F &&f) {
	auto with_axis = [&](auto ax) { if (flag) f(ax, std::true_type()); else f(ax, std::false_type()); };
	if (axis == 0u) with_axis(std::integral_constant<int, 0>()); else if (axis == 1u) with_axis(std::integral_constant<int, 1>()); else with_axis(std::integral_constant<int, 2>());
}

template <int ADDR, int LAYOUT> constexpr uint32_t variant_threads() { return LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads; }

// workgroup tiles (32 pixels wide, threads / 32 high) that cover the frame buffer shifted by the tile phase
inline void tile_grid(uint32_t out_width, uint32_t out_rows, uint32_t phase_x, uint32_t phase_y, uint32_t threads, uint32_t &tiles_x, uint32_t &tiles_y) {
	tiles_x = (out_width + phase_x + 31u) / 32u;
	tiles_y = (out_rows + phase_y + threads / 32u - 1u) / (threads / 32u);
}

// A row of select_variant's table as a value, for the callables of launch_tiles; VR_ROW_KERNEL(kernel, row) is the kernel template's instantiation for it
template <int SAMPLING, int BPV, int ADDR, int LAYOUT> struct VariantRow { static constexpr int sampling = SAMPLING, bpv = BPV, addr = ADDR, layout = LAYOUT; };
#define VR_ROW_KERNEL(kernel, row) kernel<decltype(row)::sampling, decltype(row)::bpv, decltype(row)::addr, decltype(row)::layout>
// Which rows a kernel family is instantiated for.  No run copy: a clipped composite frame and a MIP frame (launch_frame asks for none).
// The interpolated field from the copies a TRILINEAR MIP frame reads — never NEAREST, the run bricks or the voxel bricks: an isosurface
// frame and the shadowed, lit, slab and backdrop composite frames.
constexpr bool rows_all(int, int, int, int) { return true; }
constexpr bool rows_no_run(int, int, int, int layout) { return !is_run_layout(layout); }
constexpr bool rows_field(int sampling, int, int, int layout) { return sampling != VR_SAMPLE_NEAREST && !is_run_layout(layout) && layout != (int) kLayoutVoxel; }
struct NoDynamicLds { template <class Row> uint32_t operator()(Row, const RayKernelArgs &) const { return 0u; } };

// One frame of a kernel with one workgroup per screen tile — the launch sequence of every ray kernel, stated once: the row select_variant
// picks for the arguments (hipErrorInvalidValue where ROWS says the family has none), its tile grid filled into a copy of the arguments,
// dynamic_lds(row, that copy) bytes of dynamic LDS, the kernel pick(row) names, launched with (the copy, the volume copy the row reads, tail...).
template <bool (*ROWS)(int, int, int, int), class Lds, class Pick, class... Tail>
static hipError_t launch_tiles(const RayKernelArgs &args, const void *linear, const void *bricked, uint32_t bpv, hipStream_t stream,
                               Lds dynamic_lds, Pick pick, Tail... tail) {
	return select_variant(args, bricked != nullptr, bpv, [&](auto sampling, auto voxel, auto addr, auto layout, bool reads_linear) {
		constexpr int SAMPLING = decltype(sampling)::value, BPV = decltype(voxel)::value, ADDR = decltype(addr)::value, LAYOUT = decltype(layout)::value;
		if constexpr (!ROWS(SAMPLING, BPV, ADDR, LAYOUT)) return hipErrorInvalidValue;
		else {
			constexpr uint32_t threads = variant_threads<ADDR, LAYOUT>();
			constexpr VariantRow<SAMPLING, BPV, ADDR, LAYOUT> row{};
			RayKernelArgs a = args;
			tile_grid(a.p.out_width, a.p.out_rows, a.phase_x, a.phase_y, threads, a.tiles_x, a.tiles_y);
			hipLaunchKernelGGL(pick(row), dim3(a.tiles_x * a.tiles_y), dim3(threads), dynamic_lds(row, a), stream,
			                   a, reads_linear ? linear : bricked, tail...);
			return hipGetLastError();
		}
	});
}

// The frame of a composite feature family (shadowed, lit, slab, backdrop: the units beside vr_raymarch.hip, each with one launcher of
// the type CompositeLauncher, vr_device.h): the argument checks those frames share, then launch_tiles over the rows they share.
template <class Pick>
static hipError_t launch_composite_feature(const RayKernelArgs &args, const void *linear, const void *bricked, uint32_t bpv, const float *tf,
                                           const uint32_t *esl, void *out, TileSchedule sched, hipStream_t stream, Pick pick) {
	if ((args.shadow_on && args.shadow_q == 0ull) || (args.backdrop_on && (args.backdrop_rgba == 0ull || args.backdrop_depth == 0ull)) ||
	    args.p.sampling == VR_SAMPLE_NEAREST)
		return hipErrorInvalidValue;
	return launch_tiles<rows_field>(args, linear, bricked, bpv, stream, NoDynamicLds(), pick, tf, esl, (uint32_t *) out, sched.order, sched.cost);
}

}  // namespace vr
