// vr_builders.hip — what prepares a volume: the linear -> brick and column copies (LDS-tiled transposes), the feeders (per-block
// min/max, histogram) and the synthetic benchmark volumes, with their launchers.
#include "vr_march.h"

namespace vr {

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
void brick_strip_kernel(const void *__restrict__ lin, uint4 *__restrict__ out, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, uint32_t nbx, uint32_t run_cells) {
	typedef StripCfg<BPV, KIND> S;
	// run bricks: run_cells = cells a brick covers along the run axis — 8 (runs of 9 elements, 2304-byte bricks) or kRun7Cells (the aligned
	// flavour: runs of 8 elements, 2048-byte bricks; vr_device.h).  A run holds run_cells + 1 elements, the last one the next brick's first,
	// so the 9 staged slices / rows serve both.  The other kinds ignore it (8 cells per brick edge).
	constexpr bool kRun = KIND == kBuildRunZ || KIND == kBuildRunY;
	const uint32_t cells_r = kRun ? run_cells : 8u, run_len = cells_r + 1u;
	const uint32_t chunks_per_brick = kRun ? run_len * (64u * 4u / 16u) : S::chunks_per_brick;
	typedef typename VoxelT<BPV>::type V;
	__shared__ uint32_t rows[S::ny * S::nz * S::pitch_words];
	// brick order: x fastest, then the "other" axis, then the outer axis (quad / voxel / oct / runs along z: y then z; runs along y: z then y)
	const uint32_t bx0 = blockIdx.x * kStripBricks, mid = blockIdx.y, outer = blockIdx.z;
	const uint32_t y0 = KIND == kBuildRunY ? outer * cells_r : mid * 8u, z0 = KIND == kBuildRunY ? mid * 8u : outer * cells_r, x0 = bx0 * 8u;
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
	uint4 *dst = out + first_brick * chunks_per_brick;
	for (uint32_t c = t; c < bricks_here * chunks_per_brick; c += kStripThreads) {
		const uint32_t b = c / chunks_per_brick, in = c - b * chunks_per_brick, xb = b * 8u;      // brick of the strip, chunk inside it
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
				// run bricks: 64 cell columns (2-D Morton over x and the other axis) x 9 (8: aligned) elements along the run axis; the last = the next brick's first
				const uint32_t e = in * 4u + i, cell = run_len == kRun7Len ? e / kRun7Len : e / kRunLen, k = e - cell * run_len;
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
static hipError_t launch_strip(const void *linear, void *copy, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, hipStream_t stream, bool aligned_runs = false) {
	const uint32_t nbx = (dim_x + 7u) / 8u, nby = (dim_y + 7u) / 8u, nbz = (dim_z + 7u) / 8u;
	// (the aligned run bricks: ceil(n / 7) bricks along the run axis, the outer axis of the grid)
	const uint32_t run_cells = aligned_runs ? kRun7Cells : 8u, nbr = aligned_runs ? run7_bricks(KIND == kBuildRunY ? dim_y : dim_z) : (KIND == kBuildRunY ? nby : nbz);
	const dim3 grid((nbx + kStripBricks - 1u) / kStripBricks, KIND == kBuildRunY ? nbz : nby, nbr);
	hipLaunchKernelGGL((brick_strip_kernel<BPV, KIND, PLANE>), grid, dim3(kStripThreads), 0, stream, linear, (uint4 *) copy, dim_x, dim_y, dim_z, nbx, run_cells);
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
// `aligned`: the 32-byte runs of seven cells (vr_device.h kRun7*): the same kernel with 7 cells per brick along the run axis.
hipError_t launch_brickify_run(const void *linear, void *run_copy, uint32_t run_layout, bool aligned, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, hipStream_t stream) {
	if (run_layout == kLayoutRunY) return launch_strip<1, kBuildRunY, kPlaneXY>(linear, run_copy, dim_x, dim_y, dim_z, stream, aligned);
	return launch_strip<1, kBuildRunZ, kPlaneXY>(linear, run_copy, dim_x, dim_y, dim_z, stream, aligned);
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
