// vr_kernels.hip — gfx950 (CDNA4) kernels of the volume raycaster.  Written for MI355X only.
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
// Numerics.  This file is compiled with -ffp-contract=off.  NEAREST mode keeps the reference's float operation order
// expression by expression (IEEE divide / sqrt, no fused ops), so its output is bit-identical to the reference's CPU
// renderer.  TRILINEAR mode is defined with explicit fused multiply-adds (oracle/vr_oracle.c states the same sequence).
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

// RaycasterBase.h:52-65 Raycaster::sample_data_esl — bit set = block is empty; table read from LDS
__device__ __forceinline__ bool block_empty(const LdsTables &t, BlockIdx b) {
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
	constexpr bool CLIP = false;
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
	constexpr bool CLIP = true;
#include "vr_raymarch_body.inc"
}

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
// fetches from the same copy (exact, unpipelined).  Arithmetic per composited sample is the general kernel's, expression by expression.
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
__device__ __forceinline__ void col_for_window_samples(const ColBatch &b, int &pos, int cur, int bound, Refill refill, Body body) {      // body(k) for every sample of the window
	for (int batches = 0; batches < bound; batches++) {
		const int cnt = __builtin_popcountll(__builtin_amdgcn_ballot_w64(b.wvec == cur));
		for (int i = pos; i < pos + cnt; i++) body(rlane(b.kvec, i));
		pos += cnt;
		if (pos < 64) break;
		refill(); pos = 0;
	}
	pos = pos < 64 ? pos : 63;
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
	auto fetch_at = [&](float kk, uint32_t &w0, uint32_t &w1) {                           // the element pair of the sample at kk, from each lane's true column
		ColConstArgs q = col_dense_args();
		float xb, yb, zb;
		coords(q, kk, xb, yb, zb);
		const uint2 both = *(const uint2 *) col_pair_address<M>(a, ((ColConstKernelArguments) q)->copy, q->col_sample.max_x, q->col_sample.max_y, q->col_sample.max_z, q->col_shade.nbu, q->col_shade.nw, xb, yb, zb);
		w0 = both.x; w1 = both.y;
	};
	// the same as a MANAGED gather (the compiler does not see it: a load it knows to be in flight across the window loop's back edge makes
	// it put s_waitcnt vmcnt(0) in front of every window gather, and the prefetch pipeline is gone): wait with managed_wait<0>() before use
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
	// per-lane march with explicit fetches (exact, unpipelined): the few waves that straddle two kx values, and forced testing
	auto per_lane_march = [&]() {
		while (live != 0ull) {
			uint32_t w0, w1;
			fetch_at(k, w0, w1);
			sample(w0, w1);
			k += ray.step;
			live &= __builtin_amdgcn_fcmpf(k, ray.ky, kFcmpOLE);
		}
	};
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
		if (!ev.ok || (has_flips && !FLIPS)) per_lane_march();
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
	} else per_lane_march();
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
	auto per_lane_march = [&]() {                                        // exact, unpipelined: waves that straddle two kx values, forced testing
		while (live != 0ull) {
			ColConstArgs q = col_dense_args();
			const uint32_t s = *voxel_address_at(q, position(q, k));
			sample(s);
			k += ray.step;
			live &= __builtin_amdgcn_fcmpf(k, ray.ky, kFcmpOLE);
		}
	};
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
		if (!ev.ok || (has_flips && !FLIPS)) per_lane_march();
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
	} else per_lane_march();
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

	auto per_lane_march = [&]() {                                        // exact, unpipelined: waves that straddle two kx values, or too many columns
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
		// (col_bisect; the cell is monotone in k): samples with k >= t read the second column — exact per sample
		const uint32_t rw4 = (uint32_t) rw * 4u;
		const uint32_t own0 = (uint32_t) ((cu0 - ru0) + (cv0 - rv0) * rw) * 4u;
		float t_u = __builtin_inff(), t_v = __builtin_inff();
		uint32_t step_u = 0u, step_v = 0u;
		if (FLIPS && flips != 0ull) {
			const uint32_t bu = col_bisect(ray, cu0 != cu1, cu0, cell_u), bv = col_bisect(ray, cv0 != cv1, cv0, cell_v);
			t_u = cu0 != cu1 ? __uint_as_float(bu) : __builtin_inff();
			t_v = cv0 != cv1 ? __uint_as_float(bv) : __builtin_inff();
			step_u = (uint32_t) (cu1 - cu0) * 4u; step_v = (uint32_t) (cv1 - cv0) * rw4;      // (two's complement: the sums wrap back into range)
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
				col_for_window_samples(batch, pos, cur, kCells + 2, next_batch, [&](float kk) {
					k = kk;
					const uint32_t sub = (uint32_t) ((int) rfl((uint32_t) (int) VR_FMA(k, Am, Bm_l)) - first) & 15u;      // the sample's cell inside the window (uniform)
					// the owner's two slices of that cell in one dword (byte 0: slice sub, byte 1: slice sub + 1)
					const uint32_t qw = sub >> 2;
					const uint32_t lo = qw == 0u ? o.x : (qw == 1u ? o.y : (qw == 2u ? o.z : o.w));
					const uint32_t hi = qw == 0u ? o.y : (qw == 1u ? o.z : (qw == 2u ? o.w : nx));
					const int pair = (int) __builtin_amdgcn_alignbyte(hi, lo, sub & 3u);
					uint32_t at = own0;
					if (FLIPS) at += (k >= t_u ? step_u : 0u) + (k >= t_v ? step_v : 0u);
					const uint32_t p00 = (uint32_t) __builtin_amdgcn_ds_bpermute((int) at, pair), p10 = (uint32_t) __builtin_amdgcn_ds_bpermute((int) (at + 4u), pair);
					const uint32_t p01 = (uint32_t) __builtin_amdgcn_ds_bpermute((int) (at + rw4), pair), p11 = (uint32_t) __builtin_amdgcn_ds_bpermute((int) (at + rw4 + 4u), pair);
					// (u,v) (u+1,v) (u,v+1) (u+1,v+1) of slice sub -> w0, of slice sub + 1 -> w1
					const uint32_t t0 = __builtin_amdgcn_perm(p10, p00, 0x05010400u), t1 = __builtin_amdgcn_perm(p11, p01, 0x05010400u);
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

// ---- maximum-intensity projection (vr_hip_render_mip) ---------------------------------------------------------
//
// Per pixel: the ray of raymarch_kernel (get_ray, intersect), the sample sequence of its march with leaping off — k starts at kx, is
// accumulated by repeated addition of ray_step, every position is formed from k — and instead of a composite the running MAXIMUM m
// of the raw samples: NEAREST the integer voxel of Model::sample_data's unfused arithmetic, TRILINEAR the interpolated raw value
// (coordinates fma(k, A, B), the lerps of tri_resolve, Q8 weights rounded), m starting at 0.  The pixel is write_color of ONE
// transfer-function lookup of m (NEAREST transfer_fn[s8 / TF_RATIO], TRILINEAR the filtered lookup of a DVR sample), read from
// global memory once per ray: no table of it in LDS, no shading, no composite, no termination threshold.
//
// A sample is the march and the fetch.  kMipBatch samples are issued back to back before the first of them is consumed, so their
// gathers are in flight together (compiler-scheduled waits; every fetch clamps its cell like the reference, so any lane's address
// is in bounds whatever its k).  A lane fetches only while it is live AND needs the sample; a sample no lane needs issues nothing;
// the wave leaves when no lane is live.
//
// Exact acceleration (a.p.esl != 0).  m only grows, so a sample whose value cannot exceed m changes nothing:
//  * skipping: the bound of a sample is read from LDS by its ESL block index (block_index of the sample position: the grid of the
//    min/max scan).  NEAREST: the sample IS a voxel of that block, the bound is the block's maximum.  TRILINEAR: with v the voxel index
//    block_index forms per axis, the cell of the sample is floor(v - 1/2 +- rounding), i.e. v - 1 or v, its neighbour one more: the
//    eight corners lie within one voxel of the block, inside the 3x3x3 neighbouring blocks (edge >= 8 voxels) whose maximum is the
//    bound (the host keeps the frame out of this path when fp32 coordinates are not exact to a fraction of a cell: far-away views).
//    A lerp fma(t, b - a, a) with 0 <= t < 1 never leaves [min(a, b), max(a, b)], rounding included, so the interpolated value obeys
//    the bound too.  Q8 weights can round to exactly 1: the first two lerp levels are then still exact (1-byte voxels: all three —
//    every operand has at most 24 significant bits), the third may end one ulp above its larger operand for 2-byte voxels, which is
//    why that case compares against the next multiple of 256 (2-byte bounds are high bytes, padded with 0xff otherwise);
//  * stopping: once m has reached the volume's maximum the ray is finished (same bound, same argument).
// Both only skip fetches: k is advanced for every sample up to the point where the ray stops, so the image does not depend on them.
#ifndef VR_MIP_BATCH
#define VR_MIP_BATCH 4
#endif
constexpr int kMipBatch = VR_MIP_BATCH;
extern __shared__ __attribute__((aligned(16))) uint8_t mip_bound_lds[];      // kMipBoundEntries bytes of dynamic LDS, only for frames that skip

// mip_kernel and mip_clipped (a clipped frame: the segment narrowed by clip_segment) are one body, vr_mip_body.inc, compiled with CLIP = false / true
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void mip_kernel(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g, const uint8_t *__restrict__ bounds_g,
                uint32_t *__restrict__ out) {
	constexpr bool CLIP = false;
#include "vr_mip_body.inc"
}
// ... of a clipped frame (vr_hip_set_clip); a name of its own for the same reason as raymarch_clipped's
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void mip_clipped(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g, const uint8_t *__restrict__ bounds_g,
                 uint32_t *__restrict__ out) {
	constexpr bool CLIP = true;
#include "vr_mip_body.inc"
}

// block maxima of the min/max scan -> the MIP bounds (vr_device.h): one thread per block of the 32^3 grid
__global__ __launch_bounds__(256)
void mip_bounds_kernel(const uint8_t *__restrict__ minmax, uint8_t *__restrict__ bounds) {
	const uint32_t e = blockIdx.x * 256u + threadIdx.x;
	constexpr int D = VR_ESL_VOLUME_DIMS;
	const int x = (int) (e % D), y = (int) ((e / D) % D), z = (int) (e / (D * D));
	uint32_t around = 0u;
	for (int dz = -1; dz <= 1; dz++)
		for (int dy = -1; dy <= 1; dy++)
			for (int dx = -1; dx <= 1; dx++) {
				const int nx = x + dx, ny = y + dy, nz = z + dz;
				if (nx < 0 || ny < 0 || nz < 0 || nx >= D || ny >= D || nz >= D) continue;
				const uint32_t v = minmax[2 * ((nz * D + ny) * D + nx) + 1];      // unused blocks hold 0 (minmax_init_kernel)
				around = v > around ? v : around;
			}
	const uint32_t own = minmax[2 * e + 1];
	bounds[e] = (uint8_t) own;
	bounds[kMipBoundEntries + e] = (uint8_t) around;
	if (own != 0u) atomicMax((uint32_t *) (bounds + 2u * kMipBoundEntries), own);
}

hipError_t launch_mip_bounds(const uint8_t *minmax_dev, uint8_t *bounds_dev, hipStream_t stream) {
	hipError_t e = hipMemsetAsync(bounds_dev + 2u * kMipBoundEntries, 0, kMipBoundBytes - 2u * kMipBoundEntries, stream);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(mip_bounds_kernel, dim3(kMipBoundEntries / 256u), dim3(256), 0, stream, minmax_dev, bounds_dev);
	return hipGetLastError();
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
static void tile_grid(uint32_t out_width, uint32_t out_rows, uint32_t phase_x, uint32_t phase_y, uint32_t threads, uint32_t &tiles_x, uint32_t &tiles_y) {
	tiles_x = (out_width + phase_x + 31u) / 32u;
	tiles_y = (out_rows + phase_y + threads / 32u - 1u) / (threads / 32u);
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
	if (bricked != nullptr && (args.layout == kLayoutColumn || args.layout == kLayoutVoxCol)) {      // orthogonal view along args.col_axis, full march, 1-byte voxels (launch_frame)
		if (args.clip_on) return hipErrorInvalidValue;           // the column kernels march the whole cube: launch_frame takes none for a clipped frame
		RayKernelArgs a = args;
		tile_grid(a.p.out_width, a.p.out_rows, a.phase_x, a.phase_y, 512u, a.tiles_x, a.tiles_y);
		const dim3 grid(a.tiles_x * a.tiles_y), block(512);
		auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, stream, a, (const uint8_t *) bricked, tf, (uint32_t *) out); };
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

hipError_t launch_mip(const RayKernelArgs &args, const void *linear, const void *bricked, uint32_t bpv, const float *tf, const uint8_t *bounds,
                      void *out, hipStream_t stream) {
	if (args.p.esl != 0u && bounds == nullptr) return hipErrorInvalidValue;
	return select_variant(args, bricked != nullptr, bpv, [&](auto sampling, auto voxel, auto addr, auto layout, bool reads_linear) {
		constexpr int SAMPLING = decltype(sampling)::value, BPV = decltype(voxel)::value, ADDR = decltype(addr)::value, LAYOUT = decltype(layout)::value;
		if constexpr (is_run_layout(LAYOUT)) return hipErrorInvalidValue;       // a MIP frame never reads the run bricks (the caller does not ask for them)
		else {
			constexpr uint32_t threads = variant_threads<ADDR, LAYOUT>();
			RayKernelArgs a = args;
			tile_grid(a.p.out_width, a.p.out_rows, a.phase_x, a.phase_y, threads, a.tiles_x, a.tiles_y);
			// the bound table is dynamic LDS, so that frames which do not skip keep every resident workgroup the address tables allow
			const uint32_t dynamic_lds = a.p.esl != 0u ? kMipBoundEntries : 0u;
			auto kernel = a.clip_on ? mip_clipped<SAMPLING, BPV, ADDR, LAYOUT> : mip_kernel<SAMPLING, BPV, ADDR, LAYOUT>;
			hipLaunchKernelGGL(kernel, dim3(a.tiles_x * a.tiles_y), dim3(threads), dynamic_lds, stream,
			                   a, reads_linear ? linear : bricked, tf, bounds, (uint32_t *) out);
			return hipGetLastError();
		}
	});
}

// ---- shaded isosurface with depth (vr_hip_render_iso) -----------------------------------------------------------
//
// Per pixel: the ray and the sample sequence of mip_kernel's TRILINEAR march, and instead of the maximum the FIRST sample whose
// interpolated raw value reaches `level`.  The march only looks for that sample: kMipBatch fetches issued back to back, consumed in order
// behind a sched_barrier, the first one at or above the level sets hi = its k and lo = the k of the sample before it (the last k of the
// previous batch when it is the batch's first), and ends the lane; the wave leaves when no lane is live.  Everything a hit costs beyond
// that runs AFTER the loop with the wave converged again — lanes hit at different samples, inside the loop it would run once per lane:
//  * `refine` bisection steps of [lo, hi] (wave-uniform trip count, one dependent fetch each; a lane without a hit, or one that hit
//    its first sample — lo == hi —, fetches its own hi again);
//  * six clamped fetches one texel either side of the surface point, issued together: central differences scaled by N/2 are the gradient
//    in model space; the pixel is the filtered transfer-function lookup of the level times fma(kd, |n . l|, 1 - kd);
//  * one store of the pixel and, where the caller gave a buffer, one of k* (or -1).
// Every fetch clamps its cell, so no lane can form an address outside its copy whatever its k.
//
// Exact acceleration (a.p.esl != 0).  A sample whose value is below the level cannot be the first hit, so its fetch may be skipped when
// its bound — the dilated block maximum mip_kernel skips by, widened the same way (argument there) — is below the level.  That is ONE
// bit per block: the workgroup builds the 1024-word table in LDS from the byte table build_mip_bounds keeps, 4 KiB instead of mip_kernel's
// 32 KiB, and reads it with the same block index.  k advances for every sample; bisection and gradient fetches are never skipped.
extern __shared__ __attribute__((aligned(16))) uint32_t iso_skip_lds[];      // VR_ESL_VOLUME_SIZE words of dynamic LDS, only for frames that skip

// iso_kernel and iso_clipped (a clipped frame: the segment narrowed by clip_segment — a hit at its first sample is the cut face, k* = the
// clipped kx, shaded from the field's gradient there) are one body, vr_iso_body.inc, compiled with CLIP = false / true
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void iso_kernel(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g, const uint8_t *__restrict__ bounds_g,
                const float level, const uint32_t refine, uint32_t *__restrict__ out, float *__restrict__ depth) {
	constexpr bool CLIP = false;
#include "vr_iso_body.inc"
}
// ... of a clipped frame (vr_hip_set_clip); a name of its own for the same reason as raymarch_clipped's
template <int SAMPLING, int BPV, int ADDR, int LAYOUT>
__global__ __launch_bounds__(LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)>::threads)
void iso_clipped(const RayKernelArgs a, const void *__restrict__ vol, const float *__restrict__ tf_g, const uint8_t *__restrict__ bounds_g,
                 const float level, const uint32_t refine, uint32_t *__restrict__ out, float *__restrict__ depth) {
	constexpr bool CLIP = true;
#include "vr_iso_body.inc"
}

hipError_t launch_iso(const RayKernelArgs &args, const void *linear, const void *bricked, uint32_t bpv, const float *tf, const uint8_t *bounds,
                      float level, uint32_t refine, void *out_rgba, void *out_depth, hipStream_t stream) {
	if (args.p.esl != 0u && bounds == nullptr) return hipErrorInvalidValue;
	return select_variant(args, bricked != nullptr, bpv, [&](auto sampling, auto voxel, auto addr, auto layout, bool reads_linear) {
		constexpr int SAMPLING = decltype(sampling)::value, BPV = decltype(voxel)::value, ADDR = decltype(addr)::value, LAYOUT = decltype(layout)::value;
		// the interpolated field from the copies a MIP frame reads: never NEAREST (the caller refuses it), the run bricks or the voxel bricks
		if constexpr (SAMPLING == VR_SAMPLE_NEAREST || is_run_layout(LAYOUT) || LAYOUT == kLayoutVoxel) return hipErrorInvalidValue;
		else {
			constexpr uint32_t threads = variant_threads<ADDR, LAYOUT>();
			RayKernelArgs a = args;
			tile_grid(a.p.out_width, a.p.out_rows, a.phase_x, a.phase_y, threads, a.tiles_x, a.tiles_y);
			// the bit table is dynamic LDS: 4 KiB next to the address tables keep every resident workgroup frames without skipping have
			const uint32_t dynamic_lds = a.p.esl != 0u ? VR_ESL_VOLUME_SIZE * 4u : 0u;
			auto kernel = a.clip_on ? iso_clipped<SAMPLING, BPV, ADDR, LAYOUT> : iso_kernel<SAMPLING, BPV, ADDR, LAYOUT>;
			hipLaunchKernelGGL(kernel, dim3(a.tiles_x * a.tiles_y), dim3(threads), dynamic_lds, stream,
			                   a, reads_linear ? linear : bricked, tf, bounds, level, refine, (uint32_t *) out_rgba, (float *) out_depth);
			return hipGetLastError();
		}
	});
}

// ---- measured-cost tile order -------------------------------------------------------------------------------------------------
//
// The hardware starts workgroups in id order as slots free up; rays of very different length (empty-space leaping, early
// termination, rays that probe along a block face) make some tiles 10-50x longer than others, and a long tile that starts late
// IS the tail of the frame.  A frame can record what every tile cost (tile_cost: the longest wave of the tile, in 64-cycle units);
// this kernel turns that into a launch order for the next frame with the same parameters: tiles binned by cost into kOrderBins
// bins, most expensive bin first, original tile order inside a bin (neighbouring tiles of similar cost stay neighbours: they share
// cache lines).  One workgroup, a stable counting sort through LDS; clears the costs for the next recording.  Placement only.
#ifndef VR_ORDER_BINS
#define VR_ORDER_BINS 16
#endif
constexpr uint32_t kOrderBins = VR_ORDER_BINS, kOrderThreads = 512;

__global__ __launch_bounds__(kOrderThreads)
void tile_order_kernel(uint32_t *__restrict__ cost, uint32_t *__restrict__ order, uint32_t ntiles) {
	__shared__ uint32_t wave_total[kOrderBins][kOrderThreads / 64u], bin_total[kOrderBins];
	__shared__ uint32_t vmax;
	// up to kOrderCached tiles (a 2048^2 frame has 8192) the costs are read ONCE, coalesced, into LDS and the three passes below run on that
	// copy (each thread owns a contiguous run of tiles, i.e. strided global reads otherwise); larger frames read them from memory
	constexpr uint32_t kOrderCached = 8192;
	__shared__ uint32_t cached[kOrderCached];
	const uint32_t t = threadIdx.x;
	const uint32_t chunk = (ntiles + kOrderThreads - 1) / kOrderThreads, lo = t * chunk < ntiles ? t * chunk : ntiles, hi = lo + chunk < ntiles ? lo + chunk : ntiles;
	const bool in_lds = ntiles <= kOrderCached;
	if (in_lds) for (uint32_t i = t; i < ntiles; i += kOrderThreads) { cached[i] = cost[i]; cost[i] = 0; }      // (cleared for the next recording on the way)
	if (t == 0) vmax = 0;
	__syncthreads();
	auto cost_of = [&](uint32_t i) { return in_lds ? cached[i] : cost[i]; };
	uint32_t m = 0;
	for (uint32_t i = lo; i < hi; i++) { const uint32_t c = cost_of(i); m = c > m ? c : m; }
	atomicMax(&vmax, m);
	__syncthreads();
	// (bins by a float product: the 64-bit division the first version used here, twice per tile, was most of the kernel's 25 us; any
	// monotone function does as long as both passes use the same one)
	const float scale = (float) kOrderBins / ((float) vmax + 1.0f);
	auto bin_of = [&](uint32_t c) { const uint32_t q = (uint32_t) ((float) c * scale); return kOrderBins - 1u - (q < kOrderBins ? q : kOrderBins - 1u); };    // 0 = most expensive
	uint32_t mine[kOrderBins];
	for (uint32_t b = 0; b < kOrderBins; b++) mine[b] = 0;
	for (uint32_t i = lo; i < hi; i++) mine[bin_of(cost_of(i))]++;
	// exclusive scan of every bin's per-thread counts over the 512 threads: inside a wave by shuffles, across the 8 waves through LDS
	// (the first version scanned each bin serially in one thread: 22 of the kernel's 26 us)
	const uint32_t lane = t & 63u, wave = t >> 6;
	uint32_t before[kOrderBins];
	for (uint32_t b = 0; b < kOrderBins; b++) {
		uint32_t v = mine[b];
		#pragma unroll
		for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t n = __shfl_up(v, d, 64); if (lane >= d) v += n; }
		before[b] = v - mine[b];
		if (lane == 63u) wave_total[b][wave] = v;
	}
	__syncthreads();
	if (t < kOrderBins) {
		uint32_t run = 0;
		for (uint32_t w = 0; w < kOrderThreads / 64u; w++) { const uint32_t c = wave_total[t][w]; wave_total[t][w] = run; run += c; }
		bin_total[t] = run;
	}
	__syncthreads();
	uint32_t base = 0, pos[kOrderBins];
	for (uint32_t b = 0; b < kOrderBins; b++) { pos[b] = base + wave_total[b][wave] + before[b]; base += bin_total[b]; }
	for (uint32_t i = lo; i < hi; i++) { order[pos[bin_of(cost_of(i))]++] = i; }
	if (!in_lds) {
		__syncthreads();
		for (uint32_t i = lo; i < hi; i++) cost[i] = 0;
	}
}

// ---- a launch order for the FIRST frame of a policy key (round 4) ------------------------------------------------------------------
// A frame that leaps has no recorded costs yet when its view is new (the reference's benchmark renders every view once): this kernel
// predicts them.  Eight lanes per workgroup tile walk one ray each (the centres of the tile's eighths) through the 32^3 ESL bit volume in
// half-block strides and count the strides that lie in non-empty blocks: cost = the largest such count in samples + one per stride
// probed (what the ESL loop pays in empty space).  Early ray termination is not modelled (an upper estimate for opaque regions).
// Feeds tile_order_kernel like a recording does.  Placement only: the image does not depend on it.
__global__ __launch_bounds__(256)
void tile_estimate_kernel(const RayKernelArgs a, uint32_t tile_h, const uint32_t *__restrict__ esl_g, uint32_t *__restrict__ cost, uint32_t ntiles) {
	const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
	const uint32_t t = gid >> 3, probe = gid & 7u;                      // eight lanes per tile, one ray each
	uint32_t tile_x = 0, tile_y = 0;
	if (t < ntiles) tile_to_xy(a.tiles_x, a.tiles_y, t, t, tile_x, tile_y);
	const float edge = flmin(flmin(a.p.esl_block_size[0], a.p.esl_block_size[1]), a.p.esl_block_size[2]);
	uint32_t best = 0;
	do {
		if (t >= ntiles) break;
		// the centres of the tile's 4 x 2 eighths (one 8x8-pixel wave each in the 32x16 tile)
		const uint32_t px = (probe & 3u) * 8u + 4u, py = (probe >> 2) * (tile_h / 2u) + tile_h / 4u;
		const uint32_t lx = tile_x * 32u + px - a.phase_x, ly = tile_y * tile_h + py - a.phase_y;
		if (lx >= a.p.out_width || ly >= a.p.out_rows) continue;
		const PixelRay ray = pixel_ray(a, a.p.x0 + lx, frame_row(a, ly));
		if (!ray.alive) continue;
		const f3 origin = ray.origin, dir = ray.dir;
		const float kx = ray.kx, ky = ray.ky;
		const float longest = flmax(flmax(__builtin_fabsf(dir.x), __builtin_fabsf(dir.y)), __builtin_fabsf(dir.z));
		const float dk = 0.5f * edge / flmax(longest, 1e-6f);
		if (!(dk > 0.0f)) continue;
		const float strides_f = (ky - kx) / dk;
		const uint32_t strides = strides_f < 1.0f ? 1u : (strides_f > 400.0f ? 400u : (uint32_t) strides_f);
		uint32_t full = 0;
		for (uint32_t i = 0; i < strides; i++) {
			const float k = kx + ((float) i + 0.5f) * dk;
			const BlockIdx b = block_index(a, mk3(origin.x + dir.x * k, origin.y + dir.y * k, origin.z + dir.z * k));
			const uint32_t index = (b.z * VR_ESL_VOLUME_DIMS + b.y) & 0xffffu;
			if ((esl_g[index & (VR_ESL_VOLUME_SIZE - 1)] & (1u << (b.x & 31u))) == 0u) full++;
		}
		const float samples_per_stride = dk / flmax(a.p.ray_step, 1e-9f);
		const float est = (float) full * flmin(samples_per_stride, 4096.0f) + (float) strides;
		best = est > 4.0e9f ? 4000000000u : (uint32_t) est;
	} while (false);
	#pragma unroll
	for (uint32_t d = 1; d < 8u; d <<= 1) { const uint32_t o = __shfl_xor(best, d, 64); best = o > best ? o : best; }
	if (probe == 0u && t < ntiles) cost[t] = best;
}

hipError_t launch_tile_estimate(const RayKernelArgs &a, uint32_t tile_h, const uint32_t *esl, uint32_t *cost, uint32_t ntiles, hipStream_t stream) {
	hipLaunchKernelGGL(tile_estimate_kernel, dim3((ntiles * 8u + 255u) / 256u), dim3(256), 0, stream, a, tile_h, esl, cost, ntiles);
	return hipGetLastError();
}

hipError_t launch_tile_order(uint32_t *cost, uint32_t *order, uint32_t ntiles, hipStream_t stream) {
	hipLaunchKernelGGL(tile_order_kernel, dim3(1), dim3(kOrderThreads), 0, stream, cost, order, ntiles);
	return hipGetLastError();
}

// ---- choice between the two run copies per block of tiles (kLayoutRunDual) ------------------------------------------------------
// choice[t] = t, with kTileAltBit set where the frame recorded on the copy along y was cheaper than the frame recorded on the copy
// along z.  Decided per group of 64 consecutive tile numbers — one 8x8-tile block of the numbering, 256x128 pixels — from the SUMS of
// the tile costs, and for the copy along y only if it wins by 5 % (VR_DUAL_KEEP_PERCENT, tuning aid): single tile costs are noisy (they depend on what else ran on the
// CU), and tiles that read different copies share no cache lines — neighbours must agree (measured: alternating tiles +20 % frame
// time, a per-tile choice +12 % on the perspective oblique pose, where the two copies are nearly level).  Both costs NULL:
// alternating tiles (testing aid: the two copies meet at tile boundaries all over the frame).  Placement only.
__global__ __launch_bounds__(64)
void tile_choice_kernel(const uint32_t *__restrict__ cost_z, const uint32_t *__restrict__ cost_y, uint32_t *__restrict__ choice, uint32_t ntiles, uint32_t keep_percent) {
	const uint32_t t = blockIdx.x * 64u + threadIdx.x;
	bool alt;
	if (cost_z != nullptr && cost_y != nullptr) {
		uint64_t z = t < ntiles ? cost_z[t] : 0u, y = t < ntiles ? cost_y[t] : 0u;
		for (int d = 32; d >= 1; d >>= 1) { z += __shfl_xor(z, d, 64); y += __shfl_xor(y, d, 64); }
		alt = y * 100u < z * keep_percent;
	} else alt = ((t ^ (t >> 3)) & 1u) != 0u;
	if (t < ntiles) choice[t] = t | (alt ? kTileAltBit : 0u);
}

hipError_t launch_tile_choice(const uint32_t *cost_z, const uint32_t *cost_y, uint32_t *choice, uint32_t ntiles, hipStream_t stream) {
	static const uint32_t keep_percent = [] { const char *e = getenv("VR_DUAL_KEEP_PERCENT"); return e ? (uint32_t) atoi(e) : 95u; }();
	hipLaunchKernelGGL(tile_choice_kernel, dim3((ntiles + 63u) / 64u), dim3(64), 0, stream, cost_z, cost_y, choice, ntiles, keep_percent);
	return hipGetLastError();
}

// ---- linear -> brick copies: LDS-tiled streaming transposes ---------------------------------------------------------------------
//
// Every copy (quad bricks per chunk plane, voxel bricks, oct bricks, run bricks along z / y) is built by ONE kernel shape: a workgroup
// owns a STRIP of kStripBricks bricks along x — contiguous in the copy, because bricks are stored x fastest — stages the voxel rows the
// strip's elements are made of (8 x-bricks + 1 voxel wide, 8 or 9 rows x 8 or 9 slices: the +1 neighbours, indices clamped at the upper
// faces, where the interpolation weight is exactly 0) with aligned 16-byte loads into LDS, builds the elements from LDS and writes the
// strip with full 16-byte stores in copy order (256 threads x 16 bytes = 4 KiB contiguous per pass).  HBM sees the linear array about
// once (the y+1 / z+1 rows of the neighbouring strips mostly hit the L2) and the copy exactly once: bound = HBM, bytes = linear + copy.
// (Before: one thread per 4-byte element, four scattered byte loads and four byte stores each — 0.06-0.16 of the HBM peak.)
enum : int { kBuildQuad = 0, kBuildVoxel = 1, kBuildOct = 2, kBuildRunZ = 3, kBuildRunY = 4 };
constexpr uint32_t kStripBricks = 16, kStripThreads = 256;

template <int BPV, int KIND> struct StripCfg {
	static constexpr uint32_t ny = KIND == kBuildVoxel ? 8u : 9u;                                            // staged rows along y
	static constexpr uint32_t nz = (KIND == kBuildQuad || KIND == kBuildVoxel) ? 8u : 9u;                    // staged slices along z
	static constexpr uint32_t row_voxels = kStripBricks * 8u + 1u;                                           // + the x+1 neighbour of the last cell
	static constexpr uint32_t pitch_words = (row_voxels * BPV + 3u) / 4u + (((row_voxels * BPV + 3u) / 4u) % 2u == 0u ? 1u : 0u);   // odd: rows spread over the banks
	static constexpr uint32_t brick_bytes = KIND == kBuildQuad ? 512u * 4u * BPV : KIND == kBuildVoxel ? 512u * BPV : KIND == kBuildOct ? 512u * 8u * BPV : kRunBrickBytes;
	static constexpr uint32_t chunks_per_brick = brick_bytes / 16u;
};

template <int BPV, int KIND, int PLANE>
__global__ __launch_bounds__(kStripThreads)
void brick_strip_kernel(const void *__restrict__ lin, uint4 *__restrict__ out, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, uint32_t nbx) {
	typedef StripCfg<BPV, KIND> S;
	typedef typename VoxelT<BPV>::type V;
	__shared__ uint32_t rows[S::ny * S::nz * S::pitch_words];
	// brick order: x fastest, then the "other" axis, then the outer axis (quad / voxel / oct / runs along z: y then z; runs along y: z then y)
	const uint32_t bx0 = blockIdx.x * kStripBricks, mid = blockIdx.y, outer = blockIdx.z;
	const uint32_t y0 = (KIND == kBuildRunY ? outer : mid) * 8u, z0 = (KIND == kBuildRunY ? mid : outer) * 8u, x0 = bx0 * 8u;
	const uint32_t t = threadIdx.x;
	// -- stage: row (dy, dz) = voxels x0 .. x0 + 128 of line (min(y0 + dy, Y-1), min(z0 + dz, Z-1)), x clamped to X-1
	{
		const bool fast = ((uint64_t) dim_x * BPV) % 16u == 0u && (uint64_t) x0 + kStripBricks * 8u <= dim_x && ((uintptr_t) lin & 15u) == 0u;
		constexpr uint32_t vec_per_row = (kStripBricks * 8u * BPV) / 16u;                 // whole 16-byte chunks of a row (the +1 voxel comes separately)
		if (fast) {
			for (uint32_t i = t; i < S::ny * S::nz * vec_per_row; i += kStripThreads) {
				const uint32_t r = i / vec_per_row, cx = i - r * vec_per_row, dy = r % S::ny, dz = r / S::ny;
				const uint32_t y = y0 + dy < dim_y ? y0 + dy : dim_y - 1u, z = z0 + dz < dim_z ? z0 + dz : dim_z - 1u;
				const uint4 v = *(const uint4 *) ((const uint8_t *) lin + (((uint64_t) z * dim_y + y) * dim_x + x0) * BPV + (uint64_t) cx * 16u);
				uint32_t *dst = rows + r * S::pitch_words + cx * 4u;
				dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
			}
			for (uint32_t r = t; r < S::ny * S::nz; r += kStripThreads) {                 // the x+1 neighbour of the strip's last cell (clamped at the face)
				const uint32_t dy = r % S::ny, dz = r / S::ny;
				const uint32_t y = y0 + dy < dim_y ? y0 + dy : dim_y - 1u, z = z0 + dz < dim_z ? z0 + dz : dim_z - 1u;
				const uint32_t x = x0 + kStripBricks * 8u < dim_x ? x0 + kStripBricks * 8u : dim_x - 1u;
				((V *) (rows + r * S::pitch_words))[kStripBricks * 8u] = ((const V *) lin)[((uint64_t) z * dim_y + y) * dim_x + x];
			}
		} else {
			for (uint32_t i = t; i < S::ny * S::nz * S::row_voxels; i += kStripThreads) {
				const uint32_t r = i / S::row_voxels, lx = i - r * S::row_voxels, dy = r % S::ny, dz = r / S::ny;
				const uint32_t y = y0 + dy < dim_y ? y0 + dy : dim_y - 1u, z = z0 + dz < dim_z ? z0 + dz : dim_z - 1u;
				const uint32_t x = x0 + lx < dim_x ? x0 + lx : dim_x - 1u;
				((V *) (rows + r * S::pitch_words))[lx] = ((const V *) lin)[((uint64_t) z * dim_y + y) * dim_x + x];
			}
		}
	}
	__syncthreads();
	auto vox = [&](uint32_t lx, uint32_t dy, uint32_t dz) -> uint32_t { return ((const V *) (rows + (dz * S::ny + dy) * S::pitch_words))[lx]; };
	// one 32-bit word of quad element (lx, ly, lz) of slice lz: 1-byte voxels: the whole element; 2-byte: half h (0: row y, 1: row y+1)
	auto quad_word = [&](uint32_t lx, uint32_t ly, uint32_t lz, uint32_t h) -> uint32_t {
		if (BPV == 1) return vox(lx, ly, lz) | (vox(lx + 1u, ly, lz) << 8) | (vox(lx, ly + 1u, lz) << 16) | (vox(lx + 1u, ly + 1u, lz) << 24);
		return vox(lx, ly + h, lz) | (vox(lx + 1u, ly + h, lz) << 16);
	};
	const uint32_t bricks_here = nbx - bx0 < kStripBricks ? nbx - bx0 : kStripBricks;
	const uint64_t first_brick = ((uint64_t) outer * gridDim.y + mid) * nbx + bx0;
	uint4 *dst = out + first_brick * S::chunks_per_brick;
	for (uint32_t c = t; c < bricks_here * S::chunks_per_brick; c += kStripThreads) {
		const uint32_t b = c / S::chunks_per_brick, in = c - b * S::chunks_per_brick, xb = b * 8u;      // brick of the strip, chunk inside it
		uint32_t w[4];
		#pragma unroll
		for (uint32_t i = 0; i < 4u; i++) {
			uint32_t word = 0u;
			if (KIND == kBuildQuad || KIND == kBuildOct) {
				// element index inside the brick and which word of it: quad u8: 1 word per element; quad u16: 2; oct (u16): 4
				constexpr uint32_t words_per_elem = KIND == kBuildOct ? 4u : (uint32_t) BPV;
				const uint32_t local = (in * 4u + i) / words_per_elem, part = (in * 4u + i) % words_per_elem;
				const uint32_t lx = brick_collect(BPV, PLANE, 0, local), ly = brick_collect(BPV, PLANE, 1, local), lz = brick_collect(BPV, PLANE, 2, local);
				if (x0 + xb + lx < dim_x && y0 + ly < dim_y && z0 + lz < dim_z)
					word = KIND == kBuildOct ? quad_word(xb + lx, ly, lz + (part >> 1), part & 1u) : quad_word(xb + lx, ly, lz, part);
			} else if (KIND == kBuildVoxel) {
				constexpr uint32_t per_word = 4u / BPV;
				#pragma unroll
				for (uint32_t j = 0; j < per_word; j++) {
					const uint32_t local = (in * 4u + i) * per_word + j;
					const uint32_t lx = brick_collect(BPV, kPlaneXY, 0, local), ly = brick_collect(BPV, kPlaneXY, 1, local), lz = brick_collect(BPV, kPlaneXY, 2, local);
					if (x0 + xb + lx < dim_x && y0 + ly < dim_y && z0 + lz < dim_z) word |= vox(xb + lx, ly, lz) << (8u * BPV * j);
				}
			} else {
				// run bricks: 64 cell columns (2-D Morton over x and the other axis) x 9 elements along the run axis; element 8 = the next brick's first
				const uint32_t e = in * 4u + i, cell = e / kRunLen, k = e - cell * kRunLen;
				const uint32_t lx = (cell & 1u) | ((cell >> 1) & 2u) | ((cell >> 2) & 4u), lo = ((cell >> 1) & 1u) | ((cell >> 2) & 2u) | ((cell >> 3) & 4u);
				if (KIND == kBuildRunZ) {
					if (x0 + xb + lx < dim_x && y0 + lo < dim_y) word = quad_word(xb + lx, lo, k, 0u);
				} else if (x0 + xb + lx < dim_x && z0 + lo < dim_z) {           // element = the (x,z) neighbourhood of row y0 + k
					word = vox(xb + lx, k, lo) | (vox(xb + lx + 1u, k, lo) << 8) | (vox(xb + lx, k, lo + 1u) << 16) | (vox(xb + lx + 1u, k, lo + 1u) << 24);
				}
			}
			w[i] = word;
		}
		dst[c] = make_uint4(w[0], w[1], w[2], w[3]);
	}
}

template <int BPV, int KIND, int PLANE>
static hipError_t launch_strip(const void *linear, void *copy, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, hipStream_t stream) {
	const uint32_t nbx = (dim_x + 7u) / 8u, nby = (dim_y + 7u) / 8u, nbz = (dim_z + 7u) / 8u;
	const dim3 grid((nbx + kStripBricks - 1u) / kStripBricks, KIND == kBuildRunY ? nbz : nby, KIND == kBuildRunY ? nby : nbz);
	hipLaunchKernelGGL((brick_strip_kernel<BPV, KIND, PLANE>), grid, dim3(kStripThreads), 0, stream, linear, (uint4 *) copy, dim_x, dim_y, dim_z, nbx);
	return hipGetLastError();
}

hipError_t launch_brickify(const void *linear, void *bricked, uint32_t bpv, uint32_t plane, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z,
                           hipStream_t stream) {
	if (bpv == 2) return launch_strip<2, kBuildQuad, kPlaneXY>(linear, bricked, dim_x, dim_y, dim_z, stream);       // 2-byte voxels: one order (Z-order)
	if (plane == kPlaneXZ) return launch_strip<1, kBuildQuad, kPlaneXZ>(linear, bricked, dim_x, dim_y, dim_z, stream);
	if (plane == kPlaneYZ) return launch_strip<1, kBuildQuad, kPlaneYZ>(linear, bricked, dim_x, dim_y, dim_z, stream);
	return launch_strip<1, kBuildQuad, kPlaneXY>(linear, bricked, dim_x, dim_y, dim_z, stream);
}

// linear -> oct bricks (2-byte voxels): element o of the 2-byte brick order holds the 2x2x2 neighbourhood of its cell, 16 bytes
hipError_t launch_brickify_oct(const void *linear, void *oct_bricks, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, hipStream_t stream) {
	return launch_strip<2, kBuildOct, kPlaneXY>(linear, oct_bricks, dim_x, dim_y, dim_z, stream);
}

// linear -> voxel bricks: element o of the (x,y)-plane brick order holds the voxel itself (zero outside the volume)
hipError_t launch_brickify_voxel(const void *linear, void *voxel_bricks, uint32_t bpv, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, hipStream_t stream) {
	if (bpv == 1) return launch_strip<1, kBuildVoxel, kPlaneXY>(linear, voxel_bricks, dim_x, dim_y, dim_z, stream);
	return launch_strip<2, kBuildVoxel, kPlaneXY>(linear, voxel_bricks, dim_x, dim_y, dim_z, stream);
}

// linear -> run bricks (1-byte voxels): element k = 8 of a run is the first element of the next brick along the run axis (index clamped at
// the upper face, where the interpolation weight is exactly 0).  Runs along z: element = (x,y) neighbourhood of slice z; runs along y:
// element = (x,z) neighbourhood of row y.
hipError_t launch_brickify_run(const void *linear, void *run_copy, uint32_t run_layout, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, hipStream_t stream) {
	if (run_layout == kLayoutRunY) return launch_strip<1, kBuildRunY, kPlaneXY>(linear, run_copy, dim_x, dim_y, dim_z, stream);
	return launch_strip<1, kBuildRunZ, kPlaneXY>(linear, run_copy, dim_x, dim_y, dim_z, stream);
}

// ---- linear -> column windows (kLayoutColumn): LDS-tiled like the brick strips --------------------------------------------------------
// A workgroup owns NBU lateral blocks (4x4 cell columns each) side by side along u, one block row along v, and NW consecutive windows along
// the march axis m.  It stages the (4 NBU + 1) x 5 x (3 NW + 1) voxels those windows are made of (+1 neighbours, every index clamped at
// the upper faces, where the interpolation weight is exactly 0) with loads that are contiguous along x — x is u for m = y, z and the march
// axis itself for m = x, hence the two tile shapes — then writes the windows with 16-byte stores in copy order: thread t -> (block, window,
// column), 256 contiguous bytes per (block, window), a block's windows back to back.  Bound: HBM, bytes = linear + copy.
// VOX: the NEAREST windows — 16 consecutive voxels of the column itself (no +1 neighbours), cells 16w .. 16w+15, index clamped at Nm - 1.
template <int M, bool VOX> struct ColBuildCfg {
	static constexpr uint32_t cells = VOX ? kColVoxCells : kColCells;
	static constexpr uint32_t nbu = (M == 0 ? 16u : 128u) / kColEdge, nwin = M == 0 ? (VOX ? 16u : 85u) : (VOX ? 2u : 8u);        // 16 / 128 columns along u per workgroup
	static constexpr uint32_t tu = kColEdge * nbu + (VOX ? 0u : 1u), tv = kColEdge + (VOX ? 0u : 1u), te = cells * nwin + (VOX ? 0u : 1u);
	static constexpr uint32_t tx = M == 0 ? te : tu;                           // tile extent along x (the contiguous axis of the linear array)
	static constexpr uint32_t pitch = (tx + 3u) / 4u * 4u + 4u;               // bytes per staged x-row (multiple of 4, rows shifted over the banks)
	static constexpr uint32_t rows = M == 0 ? tu * tv : tv * te;              // staged rows
};

template <int M, bool VOX>
__global__ __launch_bounds__(256)
void column_build_kernel(const uint8_t *__restrict__ lin, uint4 *__restrict__ out, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z) {
	typedef ColBuildCfg<M, VOX> S;
	constexpr int U = M == 0 ? 1 : 0;
	__shared__ __attribute__((aligned(16))) uint8_t tile[S::rows * S::pitch];
	const uint32_t dim[3] = { dim_x, dim_y, dim_z };
	const uint32_t nbu = col_blocks(dim[U]), nw = col_windows(dim[M], S::cells);
	const uint32_t bu0 = blockIdx.x * S::nbu, bv = blockIdx.y, w0 = blockIdx.z * S::nwin;
	const uint32_t u0 = bu0 * kColEdge, v0 = bv * kColEdge, e0 = w0 * S::cells;
	const uint32_t t = threadIdx.x;
	// row r of the tile: m = y, z: r = dv * te + de holds u = u0 ..; m = x: r = dv * tu + du holds e = e0 ..  (x runs along the row either way)
	auto row_of = [&](uint32_t du, uint32_t dv, uint32_t de) { return M == 0 ? dv * S::tu + du : dv * S::te + de; };
	auto at = [&](uint32_t du, uint32_t dv, uint32_t de) -> uint32_t { return tile[row_of(du, dv, de) * S::pitch + (M == 0 ? de : du)]; };
	{
		const uint32_t x0 = M == 0 ? e0 : u0;
		const bool words = dim_x % 4u == 0u && ((uintptr_t) lin & 3u) == 0u;
		constexpr uint32_t wpr = (S::tx + 3u) / 4u;                           // dwords per row (the last one may be partial)
		for (uint32_t i = t; i < S::rows * wpr; i += 256u) {
			const uint32_t r = i / wpr, cw = i - r * wpr;
			uint32_t y, z;                                                    // the row's two coordinates, clamped at the upper faces
			if (M == 2) { y = v0 + r / S::te; z = e0 + r % S::te; }
			else if (M == 1) { z = v0 + r / S::te; y = e0 + r % S::te; }
			else { z = v0 + r / S::tu; y = u0 + r % S::tu; }
			y = y < dim_y ? y : dim_y - 1u; z = z < dim_z ? z : dim_z - 1u;
			const uint8_t *src = lin + ((uint64_t) z * dim_y + y) * dim_x;
			const uint32_t x = x0 + cw * 4u;
			uint32_t word;
			if (words && x + 3u < dim_x) word = *(const uint32_t *) (src + x);
			else {
				word = 0u;
				for (uint32_t j = 0; j < 4u; j++) { const uint32_t xx = x + j < dim_x ? x + j : dim_x - 1u; word |= (uint32_t) src[xx] << (8u * j); }
			}
			*(uint32_t *) (tile + r * S::pitch + cw * 4u) = word;
		}
	}
	__syncthreads();
	const uint32_t blocks_here = nbu - bu0 < S::nbu ? nbu - bu0 : S::nbu, wins_here = nw - w0 < S::nwin ? nw - w0 : S::nwin;
	constexpr uint32_t kCols = kColEdge * kColEdge;
	for (uint32_t i = t; i < blocks_here * wins_here * kCols; i += 256u) {
		const uint32_t col = i & (kCols - 1u), bw = i / kCols, w = bw % wins_here, b = bw / wins_here;
		const uint32_t du = b * kColEdge + (col & kColEdgeMask), dv = col >> kColEdgeLog2;
		uint32_t word[4];
		#pragma unroll
		for (uint32_t j = 0; j < 4u; j++) {
			if (VOX) {                                                       // dword j = voxels 16w + 4j .. + 3 of the column
				word[j] = 0u;
				#pragma unroll
				for (uint32_t b4 = 0; b4 < 4u; b4++) {
					uint32_t e = e0 + w * S::cells + j * 4u + b4;
					if (e > dim[M] - 1u) e = dim[M] - 1u;
					word[j] |= at(du, dv, e - e0) << (8u * b4);
				}
			} else {
				// element 3w + j, march index clamped at Nm - 1 (tile-relative: the staged index of the clamped element)
				uint32_t e = e0 + w * S::cells + j;
				if (e > dim[M] - 1u) e = dim[M] - 1u;
				const uint32_t de = e - e0;
				word[j] = at(du, dv, de) | (at(du + 1u, dv, de) << 8) | (at(du, dv + 1u, de) << 16) | (at(du + 1u, dv + 1u, de) << 24);
			}
		}
		out[((uint64_t) ((uint64_t) bv * nbu + bu0 + b) * nw + w0 + w) * kCols + col] = make_uint4(word[0], word[1], word[2], word[3]);
	}
}

hipError_t launch_build_column(const void *linear, void *col_copy, uint32_t axis, bool voxels, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, hipStream_t stream) {
	const uint32_t dim[3] = { dim_x, dim_y, dim_z };
	const uint32_t nbu = col_blocks(dim[col_axis_u(axis)]), nbv = col_blocks(dim[col_axis_v(axis)]), nw = col_windows(dim[axis], voxels ? kColVoxCells : kColCells);
	auto go = [&](auto kernel, uint32_t per_u, uint32_t per_w) {
		hipLaunchKernelGGL(kernel, dim3((nbu + per_u - 1u) / per_u, nbv, (nw + per_w - 1u) / per_w), dim3(256), 0, stream, (const uint8_t *) linear, (uint4 *) col_copy, dim_x, dim_y, dim_z);
	};
	dispatch_axis_flag(axis, voxels, [&](auto ax, auto vox) {
		constexpr int AX = decltype(ax)::value;
		constexpr bool VOX = decltype(vox)::value;
		go(column_build_kernel<AX, VOX>, ColBuildCfg<AX, VOX>::nbu, ColBuildCfg<AX, VOX>::nwin);
	});
	return hipGetLastError();
}

// ---- feeders: per-ESL-block min/max (RaycasterBase.cpp:101-117) as an HBM-streaming reduction --------------------------
//
// One workgroup per (y-block, z-block) pair: it streams block_dims^2 rows of dim_x voxels with 16-byte loads and keeps
// the 32 x-block minima/maxima in LDS.  min/max are order independent, so the result equals the serial scan exactly.

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

// running min / max of the 8-bit samples of one dword, two at a time in packed 16-bit lanes (v_pk_min_u16 / v_pk_max_u16)
template <int BPV>
__device__ __forceinline__ void minmax_word(uint32_t w, us2 &mn, us2 &mx) {
	if (BPV == 1) {
		const uint32_t even = w & 0x00ff00ffu, odd = (w >> 8) & 0x00ff00ffu;
		const us2 e = __builtin_bit_cast(us2, even), o = __builtin_bit_cast(us2, odd);
		mn = __builtin_elementwise_min(mn, __builtin_elementwise_min(e, o));
		mx = __builtin_elementwise_max(mx, __builtin_elementwise_max(e, o));
	} else {                                             // u16 volumes: the ESL grid works on the high byte
		const us2 h = __builtin_bit_cast(us2, (w >> 8) & 0x00ff00ffu);
		mn = __builtin_elementwise_min(mn, h);
		mx = __builtin_elementwise_max(mx, h);
	}
}

template <int BPV>
__device__ __forceinline__ void minmax_chunk(uint4 v, us2 &mn, us2 &mx) {
	minmax_word<BPV>(v.x, mn, mx); minmax_word<BPV>(v.y, mn, mx); minmax_word<BPV>(v.z, mn, mx); minmax_word<BPV>(v.w, mn, mx);
}

// One workgroup per (y-block, z-block) pair of the 32^3 ESL grid: it streams block_dims^2 rows of dim_x voxels and keeps the
// 32 x-block minima / maxima in LDS.  Three paths, same result (min / max are order independent):
//   streaming: a row is 1..256 16-byte chunks (a power of two) and every chunk lies inside one x-block — each thread owns
//              one chunk COLUMN, walks the rows with 8 independent 16-byte loads in flight, reduces in registers and touches
//              LDS once at the end.  This is the HBM-bound path (1024^3: 64 chunks per row, 4 rows per pass);
//   chunked  : 16-byte chunks inside one x-block, any row length;
//   generic  : one voxel at a time (odd dimensions, block edges that are not a multiple of the chunk).
template <int BPV>
__global__ __launch_bounds__(256)
void minmax_kernel(const void *__restrict__ vol, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, uint32_t bd,
                   uint8_t *__restrict__ minmax) {
	__shared__ uint32_t smin[VR_ESL_VOLUME_DIMS], smax[VR_ESL_VOLUME_DIMS];
	const uint32_t yb = blockIdx.x, zb = blockIdx.y;
	if (threadIdx.x < VR_ESL_VOLUME_DIMS) { smin[threadIdx.x] = 255u; smax[threadIdx.x] = 0u; }
	__syncthreads();
	const uint32_t y0 = yb * bd, z0 = zb * bd;
	const uint32_t ny = min(bd, dim_y - y0), nz = min(bd, dim_z - z0);
	const uint32_t rows = ny * nz;
	const uint64_t row_bytes = (uint64_t) dim_x * BPV;
	const uint32_t chunk_voxels = 16 / BPV;
	const bool chunked = (dim_x % chunk_voxels == 0) && (bd % chunk_voxels == 0);
	const uint32_t cpr = chunked ? dim_x / chunk_voxels : 0;          // chunks per row
	if (chunked && cpr <= 256 && (cpr & (cpr - 1)) == 0) {
		const uint32_t rows_per_pass = 256 / cpr;
		const uint32_t cx = threadIdx.x & (cpr - 1), r0 = threadIdx.x / cpr;
		us2 mn = { 255, 255 }, mx = { 0, 0 };
		auto row_ptr = [&](uint32_t row) {
			const uint32_t z = z0 + row / ny, y = y0 + row - (row / ny) * ny;
			return (const uint4 *) ((const uint8_t *) vol + ((uint64_t) z * dim_y + y) * row_bytes + (uint64_t) cx * 16);
		};
		uint32_t row = r0;
		for (; row + 7 * rows_per_pass < rows; row += 8 * rows_per_pass) {
			uint4 v[8];
			#pragma unroll
			for (int u = 0; u < 8; u++) v[u] = *row_ptr(row + u * rows_per_pass);
			#pragma unroll
			for (int u = 0; u < 8; u++) minmax_chunk<BPV>(v[u], mn, mx);
		}
		for (; row < rows; row += rows_per_pass) minmax_chunk<BPV>(*row_ptr(row), mn, mx);
		const uint32_t xb = (cx * chunk_voxels) / bd;
		atomicMin(&smin[xb], (uint32_t) min(mn.x, mn.y));
		atomicMax(&smax[xb], (uint32_t) max(mx.x, mx.y));
	} else if (chunked) {
		const uint32_t total = rows * cpr;                            // < 2^32: rows <= 2^16 * 2^16 / ... bounded by the slab size
		for (uint32_t c = threadIdx.x; c < total; c += 256) {
			const uint32_t row = c / cpr, cx = c - row * cpr;
			const uint32_t y = y0 + row % ny, z = z0 + row / ny;
			const uint8_t *p = (const uint8_t *) vol + ((uint64_t) z * dim_y + y) * row_bytes + (uint64_t) cx * 16;
			us2 mn = { 255, 255 }, mx = { 0, 0 };
			minmax_chunk<BPV>(*(const uint4 *) p, mn, mx);
			const uint32_t xb = (cx * chunk_voxels) / bd;
			atomicMin(&smin[xb], (uint32_t) min(mn.x, mn.y));
			atomicMax(&smax[xb], (uint32_t) max(mx.x, mx.y));
		}
	} else {
		const uint64_t total = (uint64_t) rows * dim_x;
		for (uint64_t i = threadIdx.x; i < total; i += 256) {
			const uint32_t row = (uint32_t) (i / dim_x), x = (uint32_t) (i - (uint64_t) row * dim_x);
			const uint32_t y = y0 + row % ny, z = z0 + row / ny;
			const uint64_t e = ((uint64_t) z * dim_y + y) * dim_x + x;
			const uint32_t s = BPV == 1 ? ((const uint8_t *) vol)[e] : (uint32_t) (((const uint16_t *) vol)[e] >> 8);
			atomicMin(&smin[x / bd], s);
			atomicMax(&smax[x / bd], s);
		}
	}
	__syncthreads();
	const uint32_t nxb = (dim_x + bd - 1) / bd;
	if (threadIdx.x < nxb && threadIdx.x < VR_ESL_VOLUME_DIMS) {
		const uint32_t e = zb * VR_ESL_VOLUME_DIMS * VR_ESL_VOLUME_DIMS + yb * VR_ESL_VOLUME_DIMS + threadIdx.x;
		minmax[2 * e] = (uint8_t) smin[threadIdx.x];
		minmax[2 * e + 1] = (uint8_t) smax[threadIdx.x];
	}
}

__global__ void minmax_init_kernel(uint8_t *minmax) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < 32u * 32u * 32u) { minmax[2 * i] = 255; minmax[2 * i + 1] = 0; }   // RaycasterBase.cpp:101-104
}

hipError_t launch_minmax(const void *volume, uint32_t bpv, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z,
                         uint32_t bd, uint8_t *minmax_dev, hipStream_t stream) {
	hipLaunchKernelGGL(minmax_init_kernel, dim3(128), dim3(256), 0, stream, minmax_dev);
	const dim3 grid((dim_y + bd - 1) / bd, (dim_z + bd - 1) / bd);
	if (bpv == 1) hipLaunchKernelGGL(minmax_kernel<1>, grid, dim3(256), 0, stream, volume, dim_x, dim_y, dim_z, bd, minmax_dev);
	else          hipLaunchKernelGGL(minmax_kernel<2>, grid, dim3(256), 0, stream, volume, dim_x, dim_y, dim_z, bd, minmax_dev);
	return hipGetLastError();
}

// ---- feeders: 256-bin histogram (ModelBase.cpp:19-26) ----------------------------------------------------------------------

// Each wave keeps kHistCopies interleaved copies of the 256 bins in LDS (bin b of copy c at b * kHistCopies + c, c = lane % 8):
// real volumes are dominated by a few values (air), and lanes that hit the same bin in one ds_add serialise — spreading them
// over 8 copies in 8 different banks cuts that 8-fold.  16-byte loads, 4 in flight per thread.
// LDS histograms per wave: lanes that count the same bin in the same instruction serialise, so every wave keeps several copies (lane & (copies - 1)).
// Measured on 1024^3 (scripts/feeder_probe.py): 1-byte voxels 3.3 / 4.0 / 4.6 / 3.1 TB/s with 4 / 8 / 16 / 32 copies, 2-byte voxels 4.7 / 4.8 / 4.4 / 4.0.
template <int BPV> struct HistCopies { static constexpr uint32_t value = BPV == 1 ? 16u : 8u; };

template <int BPV>
__global__ __launch_bounds__(256)
void histogram_kernel(const void *__restrict__ vol, uint64_t voxels, unsigned long long *__restrict__ hist) {
	constexpr uint32_t kHistCopies = HistCopies<BPV>::value;
	__shared__ uint32_t sh[4][256 * kHistCopies];
	for (uint32_t i = threadIdx.x; i < 4 * 256 * kHistCopies; i += 256) ((uint32_t *) sh)[i] = 0;
	__syncthreads();
	uint32_t *mine = sh[threadIdx.x >> 6] + (threadIdx.x & (kHistCopies - 1));
	auto count = [&](uint32_t bin) { atomicAdd(&mine[bin * kHistCopies], 1u); };
	auto chunk = [&](uint4 v) {
		const uint32_t w[4] = { v.x, v.y, v.z, v.w };
		#pragma unroll
		for (int i = 0; i < 4; i++) {
			if (BPV == 1) { count(w[i] & 0xffu); count((w[i] >> 8) & 0xffu); count((w[i] >> 16) & 0xffu); count(w[i] >> 24); }
			else          { count((w[i] >> 8) & 0xffu); count(w[i] >> 24); }          // u16: high byte
		}
	};
	const uint64_t stride = (uint64_t) gridDim.x * 256;
	const uint64_t vec = voxels * BPV / 16;              // whole 16-byte chunks
	uint64_t c = (uint64_t) blockIdx.x * 256 + threadIdx.x;
	for (; c + 3 * stride < vec; c += 4 * stride) {
		const uint4 v0 = ((const uint4 *) vol)[c], v1 = ((const uint4 *) vol)[c + stride];
		const uint4 v2 = ((const uint4 *) vol)[c + 2 * stride], v3 = ((const uint4 *) vol)[c + 3 * stride];
		chunk(v0); chunk(v1); chunk(v2); chunk(v3);
	}
	for (; c < vec; c += stride) chunk(((const uint4 *) vol)[c]);
	if (blockIdx.x == 0) {                               // tail (fewer than 16 bytes)
		const uint64_t done = vec * 16 / BPV;
		for (uint64_t i = done + threadIdx.x; i < voxels; i += 256)
			count(BPV == 1 ? ((const uint8_t *) vol)[i] : (uint32_t) (((const uint16_t *) vol)[i] >> 8));
	}
	__syncthreads();
	const uint32_t b = threadIdx.x;
	unsigned long long sum = 0;
	for (uint32_t w = 0; w < 4; w++)
		for (uint32_t cp = 0; cp < kHistCopies; cp++) sum += sh[w][b * kHistCopies + cp];
	if (sum) atomicAdd(&hist[b], sum);
}

hipError_t launch_histogram(const void *volume, uint32_t bpv, uint64_t voxels, unsigned long long *hist, hipStream_t stream) {
	hipError_t e = hipMemsetAsync(hist, 0, 256 * sizeof(unsigned long long), stream);
	if (e != hipSuccess) return e;
	// each workgroup may add at most 2^32-1 per bin into its LDS counters: bound the voxels per workgroup
	uint64_t blocks = (voxels + (1ull << 24) - 1) >> 24;
	if (blocks < 2048) blocks = 2048;
	if (bpv == 1) hipLaunchKernelGGL(histogram_kernel<1>, dim3((uint32_t) blocks), dim3(256), 0, stream, volume, voxels, hist);
	else          hipLaunchKernelGGL(histogram_kernel<2>, dim3((uint32_t) blocks), dim3(256), 0, stream, volume, voxels, hist);
	return hipGetLastError();
}

// ---- synthetic benchmark volumes, integer-only, generated straight into HBM --------------------------------

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
	h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
	return h;
}

// One thread per 16-byte chunk of the array (16 or 8 consecutive voxels along x, wrapping into the next row / slice), one 16-byte store.
// The shell's 1000 * d2 / (N * N) is an exact integer quotient (< 12000): a shift where N is a power of two, else formed in DOUBLE
// precision (every quantity is an integer below 2^53 for n <= 65535, so the fused remainder r = num - q * N^2 is exact and the estimate
// floor(num / N^2) is corrected by its sign) — the 64-bit integer division it replaces was what the old one-voxel-per-thread kernel
// spent its time in.  What remains is the murmur finaliser per voxel: the kernel is bound by integer issue, not by HBM.
// `shift` != 0: n is a power of two, n * n = 1 << shift, and the quotient is a 64-bit multiply and a shift (the benchmark sizes).
// The shell is zero wherever 1000 * d2 / n^2 lies outside (120, 600): |q - 360| >= 240.
template <int BPV>
__device__ __forceinline__ uint32_t synthetic_voxel(uint32_t kind, uint64_t idx, int ax, uint64_t ayz2, double nn, double inv_nn, uint32_t shift, uint32_t seed) {
	const uint32_t h = fmix32((uint32_t) (idx ^ (idx >> 32)) + seed * 0x9E3779B9u);
	if (kind != 0) return h & 255u;
	const uint64_t num = 1000ull * ((uint64_t) ((int64_t) ax * ax) + ayz2);   // < 2^53 for every n <= 65535
	int q;
	if (shift != 0u) q = (int) (num >> shift);
	else {
		double e = __builtin_floor((double) num * inv_nn);
		const double r = __builtin_fma(-e, nn, (double) num);        // exact remainder of the estimate (every quantity is an integer < 2^53)
		if (r < 0.0) e -= 1.0; else if (r >= nn) e += 1.0;
		q = (int) e;
	}
	int t = q - 360;
	if (t < 0) t = -t;
	int shell = 255 - (int) ((uint32_t) t * 255u / 240u);
	if (shell < 0) shell = 0;
	const uint32_t v = (uint32_t) shell + (h & 15u);
	return v > 255u ? 255u : v;
}

template <int BPV>
__global__ __launch_bounds__(256)
void generate_kernel(void *__restrict__ vol, uint32_t kind, uint32_t n, uint32_t seed) {
	constexpr uint32_t kPerChunk = 16u / BPV;
	const int N = (int) n;
	const double nn = (double) n * (double) n, inv_nn = 1.0 / nn;
	const uint32_t shift = (n & (n - 1u)) == 0u ? 2u * (uint32_t) __builtin_ctz(n) : 0u;
	const uint64_t total = (uint64_t) n * n * n, chunks = total / kPerChunk;
	const uint64_t stride = (uint64_t) gridDim.x * 256;
	for (uint64_t c = (uint64_t) blockIdx.x * 256 + threadIdx.x; c < chunks; c += stride) {
		uint64_t idx = c * kPerChunk;
		const uint64_t row = idx / n;
		uint32_t x = (uint32_t) (idx - row * n), y = (uint32_t) (row % n), z = (uint32_t) (row / n);
		int64_t ay = 2 * (int64_t) y + 1 - N, az = 2 * (int64_t) z + 1 - N;
		uint64_t ayz2 = (uint64_t) (ay * ay + az * az);
		uint32_t w[4] = { 0u, 0u, 0u, 0u };
		#pragma unroll
		for (uint32_t j = 0; j < kPerChunk; j++) {
			const uint32_t v = synthetic_voxel<BPV>(kind, idx, 2 * (int) x + 1 - N, ayz2, nn, inv_nn, shift, seed);
			if (BPV == 1) w[j / 4u] |= v << (8u * (j % 4u)); else w[j / 2u] |= (v * 257u) << (16u * (j % 2u));
			idx++;
			if (++x == n) {                                       // next row (and slice)
				x = 0;
				if (++y == n) { y = 0; z++; az = 2 * (int64_t) z + 1 - N; }
				ay = 2 * (int64_t) y + 1 - N; ayz2 = (uint64_t) (ay * ay + az * az);
			}
		}
		((uint4 *) vol)[c] = make_uint4(w[0], w[1], w[2], w[3]);
	}
	if (blockIdx.x == 0) {                                           // fewer than 16 bytes left over
		for (uint64_t idx = chunks * kPerChunk + threadIdx.x; idx < total; idx += 256) {
			const uint64_t row = idx / n;
			const int x = (int) (idx - row * n);
			const int64_t ay = 2 * (int64_t) (row % n) + 1 - N, az = 2 * (int64_t) (row / n) + 1 - N;
			const uint32_t v = synthetic_voxel<BPV>(kind, idx, 2 * x + 1 - N, (uint64_t) (ay * ay + az * az), nn, inv_nn, shift, seed);
			if (BPV == 1) ((uint8_t *) vol)[idx] = (uint8_t) v; else ((uint16_t *) vol)[idx] = (uint16_t) (v * 257u);
		}
	}
}

hipError_t launch_generate(void *volume, uint32_t kind, uint32_t n, uint32_t seed, uint32_t bpv, hipStream_t stream) {
	if (bpv == 1) hipLaunchKernelGGL(generate_kernel<1>, dim3(8192), dim3(256), 0, stream, volume, kind, n, seed);
	else          hipLaunchKernelGGL(generate_kernel<2>, dim3(8192), dim3(256), 0, stream, volume, kind, n, seed);
	return hipGetLastError();
}

}  // namespace vr
