// vr_device.h — launch interface between the C ABI (vr_hip_api.cpp) and the gfx950 kernel units (vr_raymarch.hip, vr_project.hip,
// vr_kernels.hip, vr_schedule.hip, vr_builders.hip; what they share among themselves is vr_march.h).
// Internal to libvr_hip.so; the public boundary is include/vr_hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/vr_hip.h"

namespace vr {

// Hang guard: no ray of any reference view needs more than ~3.5 / ray_step iterations (k spans at most the cube
// diagonal, 2*sqrt(3), in units of |direction| >= 1).  A ray that would exceed this many iterations of either loop
// is cut off instead of stalling the GPU (k += ray_step stops advancing once k >= 2^24 * ray_step).
constexpr uint32_t kMaxRaySteps = 1u << 22;

// Software pipeline of the march: the gathers of sample i + kDepth are issued before sample i is consumed; the loop body is
// instantiated once per fetch slot (kDepth + 1 of them, rotating roles — no register copies) and iteration.  A finished lane has
// up to kDepth speculative fetches beyond its exit point, which the kLutPad repeated edge entries of the address tables absorb:
// the host checks kOverrunSteps * (cells per step) + 1.5 <= kLutPad per frame and otherwise runs the coordinate-clamping variant.
#ifndef VR_DEPTH
#define VR_DEPTH 5
#endif
constexpr int kDepth = VR_DEPTH, kSlots = kDepth + 1;
// Lazy exit test (unclamped march): whether a lane has left its ray segment is tested once per rotation of the fetch slots (and by
// every sample that composites), not per sample — a finished lane then marches up to kSlots further steps before its step becomes 0.
#ifndef VR_LAZY_EXIT
#define VR_LAZY_EXIT 1
#endif
// prefetch depth of the run-brick variants (one 8-byte gather = two registers per slot)
#ifndef VR_RUN_DEPTH
#define VR_RUN_DEPTH VR_DEPTH
#endif
constexpr int kDepthTwoByte = 3;        // TRILINEAR with 2-byte voxels: four registers per slot — three samples ahead keep 64 VGPRs
constexpr int kRunDepth = VR_RUN_DEPTH, kMaxDepth = kRunDepth > kDepth ? kRunDepth : kDepth;
constexpr int kOverrunSteps = kMaxDepth + (VR_LAZY_EXIT ? kMaxDepth + 1 : 0);     // steps a speculative fetch may lie beyond a ray's exit point
constexpr int kLutPad = (kOverrunSteps * 5 + 2) / 3 + 2;                          // >= kOverrunSteps * 1.666 (the reference's longest step, in cells) + 1.5
static_assert(kDepth >= 1 && kDepth <= 6 && kRunDepth >= 1 && kRunDepth <= 12, "prefetch depth");

// Everything the ray-march kernel reads that is not an array: passed BY VALUE as the kernel argument (the reference
// does the same with its Raycaster POD, GPURenderer1.cu:30,108) so it lands in SGPRs via s_load from the kernarg segment.
struct RayKernelArgs {
	vr_params p;
	uint32_t dim_x, dim_y, dim_z;      // Model::dims (ModelBase.h:13), widened
	uint32_t tiles_x, tiles_y;         // workgroup tiles (32x16 or 32x32 pixels) over the output; filled in at launch
	uint32_t phase_x, phase_y;         // the tile grid starts at pixel (-phase_x, -phase_y) of the output buffer (0..7)
	uint32_t lane_map;                 // order of the 16 lanes of a 4x4-pixel group: kLaneRows (4 consecutive lanes = 4 pixels along
	                                   // screen x), kLaneColumns (along screen y), kLaneBlocks (2x2-pixel blocks)
	uint64_t stride_y, stride_z;       // voxel strides (elements): dim_x, dim_x*dim_y
	float    half_x, half_y, half_z;   // 0.5f * dim  (TRILINEAR coordinate: xb = fma(pos, half, half - 0.5))
	float    off_x,  off_y,  off_z;    // 0.5f * dim - 0.5f
	float    max_x,  max_y,  max_z;    // dim - 1 as float (clamp addressing)
	float    lh_x,   lh_y,   lh_z;     // 0.01f * half: texel-space length of the shading offset (GPURenderer4.cu:43-46)
	float    tf_scale;                 // 128/255 (u8) or 128/65535 (u16): raw interpolated voxel -> TF texel coordinate + 0.5
	float    kd_scaled;                // light_kd / 255 (u8) or / 65535 (u16)
	float    tf_zero_below;            // entries 0..tf_zero_below of the premultiplied TF are exactly (0,0,0,0); -1 if entry 0 is not
	uint32_t skip_mask;                // per-voxel bit mask ~(skip_below - 1), replicated over the packed word: all 8 corners below the
	                                   // power of two skip_below => TF coordinate <= tf_zero_below
	uint32_t skip_cmp;                 // the corner test is (corners & skip_mask) != skip_cmp: 0 normally; a TF with no leading zero entries
	                                   // (no sample may take the shortcut) sets skip_mask = 0, skip_cmp = 1 — the test then always holds
	uint32_t clamp_fetch;              // 1: clamp the fetch coordinates of every sample (views whose fp32 coordinates may leave (-1, N),
	                                   // ray steps so long that two of them leave the table padding)
	uint32_t near_scaled;              // 1: every edge is a power of two — NEAREST may march in the scaled domain (sample_nearest_scaled)
	uint32_t esl_div_magic, esl_div_shift;   // n / esl_block_dims: magic != 0 ? mulhi(n, magic) : n >> shift
	uint32_t layout;                   // vr_layout in use for this launch
	uint32_t brick_plane;              // chunk plane of the brick copy handed to the kernel (kPlaneXY ...)
	uint32_t force_wide;               // testing aid: 1 = arithmetic 64-bit path, 2 = 64-bit table path, even for small volumes
	uint32_t nbx, nby, nbz;            // bricks per axis (bricked layout)
	uint64_t alt_copy;                 // kLayoutRunDual: address of the run copy along y (the kernel's `vol` argument is the copy along z)
	                                   // kLayoutVoxCol: the quad-element windows of the march axis (kCopyColX ..) that voxcol_pairs_kernel shades from, or 0
	uint32_t dual_analytic;            // kLayoutRunDual: 1 = every tile picks its run copy from dual_bits (no launch-order entry needed)
	uint32_t dual_shift;               // ... one bit per group of (1 << dual_shift) consecutive tile NUMBERS (>= 6: 64 numbers = one 8x8-tile block of the numbering)
	uint32_t dual_bits[32];            // ... bit set = the block's tiles read the copy with runs along y (vr_hip_api.cpp dual_choice_bits)
	uint32_t col_axis;                 // kLayoutColumn: the march axis m (0 x, 1 y, 2 z) of the window copy handed to the kernel
	// kLayoutColumn: what the DENSE path of the column kernels reads back from the kernel-argument segment (it cannot keep these ~25 scalars
	// live across the march), grouped so that ONE scalar load fetches everything a step of that path needs: the path is a dependent chain
	// per wave, and every separate s_load + s_waitcnt on it is a scalar-cache round trip (seven of them per shaded sample before the grouping)
	struct ColDenseSample {            // every composited sample
		float ax, ay, az;              // direction * half (the texel-space direction A of coordinate = fma(k, A, B)), the device's own fp32 products
		float tf_scale;
		float max_x, max_y, max_z;
		float tf_zero_below;
		float light_kd, ray_threshold;
		uint32_t pad[2];
	} col_sample;
	struct ColDenseShade {             // samples that are shaded
		float dir[3];  float kd_scaled;
		float light[3]; uint32_t nbu;  // lateral blocks along u (col_blocks(dim_u))
		float lh[3];   uint32_t nw;    // windows per column (col_windows(dim_m))
		uint32_t dim[3], nwq;          // Model::dims (colmarch_nearest_kernel: map_float_int of the shading position); windows per column of the
		                               // quad-element copy at alt_copy (voxcol_pairs_kernel: nw is then the voxel windows')
	} col_shade;
	// vr_hip_set_clip (include/vr_hip.h vr_clip): the crop box and the kept half-space of a clipped frame.  Read by the
	// *_clipped kernels only (vr_march.h clip_segment) — the kernels of unclipped frames never look at these words; clip_on is for the host
	uint32_t clip_on;
	float    clip_min[3], clip_max[3], clip_plane[4];
	// vr_hip_set_shadow (include/vr_hip.h vr_shadow): the light grid a shadowed composite frame scales its dense samples
	// by.  Read by the raymarch_shadowed kernels only, through the laundered kernel-argument pointer like the clip words; shadow_on is for the
	// host.  Such a frame always runs clip_segment: without a clip the host fills the identity clip above, which changes no bit.
	uint32_t shadow_on;
	uint32_t shadow_last;              // S - 2: the highest cell index per axis
	float    shadow_hs;                // 0.5f * (S - 1): node coordinate = fma(pt, hs, hs)
	float    shadow_max;               // (float) (S - 1)
	float    shadow_scale;             // strength * (1.0f / 255.0f)
	float    shadow_base;              // 1.0f - strength
	uint32_t shadow_row, shadow_slab;  // S, S * S: byte strides of the plain array along y and z
	uint64_t shadow_q;                 // the S^3 bytes q, x fastest
	// vr_hip_set_lighting (include/vr_hip.h vr_lighting): the Blinn-Phong constants of a gradient-lit composite frame.
	// Read by the composite_lit kernels only (vr_light.hip), inside their dense block through the laundered kernel-argument pointer
	// (vr_march.h light_sample), so nothing of them is live across the march; light_on is for the host.  Such a frame always runs clip_segment
	// (the identity clip above when none is set) and applies shadow_factor when shadow_on is set: the two compose.
	uint32_t light_on;
	float    light_ka, light_kd, light_ks;
	uint32_t light_n;                  // shininess_log2: the specular term is squared this many times
#ifdef VR_BOUNDS_CHECK
	// `make EXTRA=-DVR_BOUNDS_CHECK` (debug build, not the product): every gather address of the march is held against the array it must
	// lie in, every address-table index against its padded table, the tile-cost slot against its buffer; the first violation is recorded
	// in bc_fault[0..5] = { code, workgroup, thread, value lo, value hi, limit } and the access is redirected to the start of the array,
	// so the frame completes and the launch returns VR_ERR_HIP instead of faulting the GPU.
	uint64_t bc_base, bc_bytes;        // the array `vol` points at (brick copy or linear array incl. tail slack)
	uint64_t bc_alt_bytes;             // kLayoutRunDual: size of the copy at alt_copy
	uint32_t *bc_fault;
	uint32_t bc_ntiles;
#endif
	// vr_hip_set_preintegration (include/vr_hip.h): 1 = slab classification.  For the host alone (launch_raymarch
	// hands such a frame to vr_slab.hip); no kernel reads it.  The table K lies behind the 128 entries of the transfer function.
	uint32_t slab_on;
	// vr_hip_render_backdrop (include/vr_hip.h vr_backdrop): the opaque layer a backdrop frame stops at and blends over.
	// Read by the composite_backdrop* kernels only (vr_backdrop.hip, vr_backdrop_slab.hip), through the laundered kernel-argument pointer like
	// the clip words: the depth in front of the march, the colour (and the depth again) behind it.  Addresses, not pointers: the output buffer
	// may be the colour layer.  backdrop_on is for the host (launch_raymarch hands such a frame to the new units).
	uint32_t backdrop_on;
	// The flavour of the run bricks a run-layout frame reads: 1 = `vol` / alt_copy are the ALIGNED run bricks (kCopyRun7Z / Y: 32-byte runs
	// of seven cells), 0 = the 36-byte runs.  Wave-uniform; read by the table staging of the run layouts only.  HERE because these four bytes
	// were alignment padding: no other member moves and the argument keeps its size, so no other kernel's loads change.
	uint32_t run_aligned;
	uint64_t backdrop_rgba, backdrop_depth;
};
// Tiles are numbered in VR_TILE_ORDER x VR_TILE_ORDER blocks (blocks row-major, tiles column by column inside a block — VR_XCD_MODE
// below —, the ragged right / bottom margins after them): consecutive workgroups — which the hardware spreads over the eight XCDs — are screen neighbours.
#ifndef VR_TILE_ORDER
#define VR_TILE_ORDER 8
#endif
// Which tiles of an 8x8-tile block share an XCD (vr_march.h tile_to_xy, measurements there): 5 = the tiles of a block are numbered
// column by column, so that in workgroup order XCD x renders ROW x of every block.
#ifndef VR_XCD_MODE
#define VR_XCD_MODE 5
#endif
// tile number -> tile column / row; what raymarch_kernel computes (without its other experiment switches), for the host (cost map)
inline void tile_number_to_xy(uint32_t tile, uint32_t tiles_x, uint32_t tiles_y, uint32_t *x, uint32_t *y) {
	constexpr uint32_t B = VR_TILE_ORDER > 1 ? VR_TILE_ORDER : 1;
	const uint32_t full_cols = tiles_x / B, full_rows = tiles_y / B, nblocked = full_cols * full_rows * B * B;
	if (tile < nblocked) {
		const uint32_t blk = tile / (B * B), in = tile - blk * (B * B), by = blk / full_cols, bx = blk - by * full_cols;
		if (B == 8 && VR_XCD_MODE == 5) { *x = bx * B + in / B; *y = by * B + in % B; }
		else { *x = bx * B + in % B; *y = by * B + in / B; }
		return;
	}
	uint32_t rest = tile - nblocked;
	const uint32_t right_w = tiles_x - full_cols * B, right_n = right_w * full_rows * B;
	if (rest < right_n) { *y = rest / right_w; *x = full_cols * B + rest % right_w; }
	else { rest -= right_n; *y = full_rows * B + rest / tiles_x; *x = rest % tiles_x; }
}

// measured-cost launch order of a frame (vr_schedule.hip tile_order_kernel): order = workgroup id -> tile number or NULL (identity);
// cost = per tile, the longest wave of the tile in 64-cycle units, or NULL (not recorded)
struct TileSchedule { const uint32_t *order = nullptr; uint32_t *cost = nullptr; };

// TRILINEAR volume layouts.
//   kLayoutLinear : the reference's x-fastest array (+ zeroed tail slack); a sample = 4 two-voxel loads at VOXEL
//                   alignment.  Measured on MI355X (scripts/ubench/vmem_rate.hip): a 2-byte load at an odd address costs
//                   4x an aligned one, and a wave that touches n cache lines pays ~n cycles in the L1 tag pipe.
//   kLayoutBricked: "quad bricks".  Element (x,y,z) packs the 2x2 (x,y) neighbourhood {v(x,y), v(x+1,y), v(x,y+1),
//                   v(x+1,y+1)} of slice z (indices clamped at the upper faces, where the weight is exactly 0) into one
//                   naturally ALIGNED 4-byte (u8) / 8-byte (u16) word.  Elements are stored in bricks of 8x8x8 positions;
//                   the order inside a brick is kBrickBits below.  A trilinear sample is TWO aligned loads (slices z and
//                   z+1); the vector memory pipeline serves a gather one lane quad at a time and is fastest when the
//                   quad's four addresses share an aligned 16-byte chunk (scripts/ubench/tcp_coalesce.hip), which is
//                   what the brick order and the lane order of the ray-march kernel are chosen for.  Costs 4x the voxel
//                   bytes in HBM.
//   kLayoutRun    : "run bricks" — the same quad elements, but the 8 elements of a cell column (x,y) inside a brick are
//                   CONTIGUOUS along z and followed by a duplicate of the next brick's first one (9 x 4 = 36 bytes), so that the
//                   slices z and z+1 of ANY sample are 8 adjacent bytes: ONE global_load_dwordx2 (4-byte aligned) per sample.
//                   Measured (scripts/ubench/tcp_gather64.hip): for lane quads that straddle chunks — every view that is not
//                   along a volume axis — one such gather costs 8-9 ns per wave against 2 x 7-9 ns for the two 4-byte gathers;
//                   for the chunk-aligned quads of axis-aligned views the two 4-byte gathers are cheaper (2 x 1.9 ns against
//                   6.8), so this copy is read by oblique views only.  9/8 of a quad copy, 64-bit addresses (4.5 GiB at 1024^3).
//   kLayoutRunY   : run bricks whose runs lie along Y: the element is the 2x2 neighbourhood in the (x,z) plane of row y, the 9-element
//                   runs hold rows y .. y+8 of a cell column (x,z).  Same single 8-byte gather; read by the views that march
//                   mostly along z, for which the runs of kLayoutRun would lie ALONG the march (measured: perspective along z
//                   2.99 ms with runs along z against 2.47 ms with the quad copy) — runs should lie across it.
//   kLayoutVoxel  : "voxel bricks" for NEAREST sampling — ONE voxel per element in the brick order of the (x,y) quad copy.  NEAREST
//                   needs one voxel per sample; reading it out of a 4-byte quad element moves 4x the bytes and makes a 16-byte
//                   chunk cover 2x2 cells.  With 1-byte elements a chunk covers 4x4 cells of a slice and a 128-byte line 8x8x2
//                   voxels: the lane quads of views that are not aligned stay inside one chunk far more often, and the
//                   compulsory traffic of a frame is the volume itself (1 GiB at 1024^3).
//   kLayoutOct    : "oct bricks" for TRILINEAR sampling of 2-BYTE voxels — element (x,y,z) is the whole 2x2x2 neighbourhood, eight
//                   2-byte voxels = ONE aligned 16-byte word, in the brick order of the 2-byte quad copy.  Measured
//                   (scripts/ubench/tcp_gather64.hip, column "u16 oct"): an aligned 16-byte gather costs what ONE 8-byte gather costs
//                   (6.7-10 ns per wave in every lane pattern), and the quad bricks need two of those per sample.  Twice the bytes of
//                   the quad copy (16 per voxel: 128 GiB for 2048^3); for 1-byte voxels the same idea (8-byte octets) lost against
//                   the run bricks, which share their elements along z.
//   kLayoutRunDual: BOTH run copies in one launch, chosen per screen tile (bit 31 of the tile's entry in the launch order: 0 = runs
//                   along z, 1 = runs along y).  For a view that is not along an axis the better copy depends on the cube face a tile's
//                   rays enter through: all lanes of a wave start ON that face and march in lockstep, so the wave's 64 samples lie in a
//                   plane parallel to it — with runs perpendicular to that plane no two lanes share a run (measured per tile on the
//                   oblique benchmark pose: the upper half of the screen is 25 % cheaper with runs along y, the lower half with runs
//                   along z).  The host measures both copies per tile on the first two frames of a parameter set (vr_hip_api.cpp).
//   kLayoutColumn : "column windows" (round 4) for ORTHOGONAL views along a volume axis m, full march.  Every ray of such a view stays in
//                   one cell column (u,v) for its whole march (but for at most one cell flip per lateral axis when the direction carries
//                   rounding noise), and all rays share one k sequence, so the cell ALONG the march is the same for the whole wave at
//                   every sample.  The copy holds, per cell column, WINDOWS of four consecutive quad elements along m (element e =
//                   the 2x2 (u,v) neighbourhood at march index min(e, Nm-1); window w = elements 3w .. 3w+3 = the three cells
//                   3w .. 3w+2) as ONE aligned 16-byte word; the 4x4 columns of a lateral block are contiguous (256 bytes) and a
//                   block's windows follow each other along m: address = ((bv * nbu + bu) * nw + w) * 256 + (v & 3) * 64 + (u & 3) * 16.
//                   One 16-byte gather serves the ~3 samples of a window, its transparency test is done once for the window, and the
//                   address chain of a sample shrinks to the wave-uniform cell along m (colmarch_kernel).  16/3 bytes per voxel.
//   kLayoutVoxCol : the column-march views and the TRILINEAR arithmetic of kLayoutColumn, read from the NEAREST windows of 16 plain voxels
//                   (kCopyColVox*, 1 byte per voxel): a wave gathers the rectangle of cell columns its lanes sample, one column per
//                   lane, and hands every lane its 2x2 corner columns by cross-lane permutes (voxcol_tri_kernel).  Taken where the host
//                   can bound that rectangle to 64 columns (vr_hip_api.cpp), kLayoutColumn otherwise.  A LIT frame fetches its shading
//                   samples (positions off the wave's rectangle) from the quad-element windows of the same axis, one 8-byte load instead
//                   of eight byte loads (voxcol_pairs_kernel), when that copy can be had too.
enum : uint32_t { kLayoutLinear = 0, kLayoutBricked = 1, kLayoutRun = 2, kLayoutRunY = 3, kLayoutVoxel = 4, kLayoutOct = 5, kLayoutRunDual = 6, kLayoutColumn = 7,
                  kLayoutVoxCol = 8 };
__host__ __device__ constexpr bool is_run_layout(int layout) { return layout == (int) kLayoutRun || layout == (int) kLayoutRunY || layout == (int) kLayoutRunDual; }
constexpr uint32_t kDualWords = 32;
constexpr uint32_t kTileAltBit = 0x80000000u;       // kLayoutRunDual: set in a launch-order entry = this tile reads the copy with runs along y
__host__ __device__ constexpr bool is_brick_table_layout(int layout) { return layout == (int) kLayoutBricked || layout == (int) kLayoutVoxel; }
constexpr uint32_t kRunLen = 9, kRunBytes = kRunLen * 4, kRunBrickBytes = 64 * kRunBytes;       // 8x8 cell columns per brick
// byte offset of cell column (x & 7, y & 7) inside a run brick: 2-D Morton order, 36-byte runs
__host__ __device__ inline uint32_t run_cell_order(uint32_t axis, uint32_t v) {       // ... the column's place in that order (both flavours)
	return ((v & 1u) << axis) | (((v >> 1) & 1u) << (2 + axis)) | (((v >> 2) & 1u) << (4 + axis));
}
__host__ __device__ inline uint32_t run_cell_spread(uint32_t axis, uint32_t v) { return run_cell_order(axis, v) * kRunBytes; }
inline uint64_t run_copy_bytes(uint32_t dim_x, uint32_t dim_y, uint32_t dim_z) {
	return (uint64_t) ((dim_x + 7) / 8) * ((dim_y + 7) / 8) * ((dim_z + 7) / 8) * kRunBrickBytes + 16;
}
// The second flavour of the run bricks, "aligned runs" (kCopyRun7Z / kCopyRun7Y): a run is 8 elements = 32 bytes and covers SEVEN cells
// along the run axis — element 7 duplicates the next brick's first, as element 8 does above — so a brick of 8x8 cell columns is 2048
// bytes, the run axis has ceil(n / 7) bricks, no run straddles a 128-byte line and every line is one 2x2 block of cell columns (the same
// 2-D Morton order) x 7 cells; a slice pair straddles a 16-byte chunk in 1 of 7 positions instead of 1 of 4.  32/7 bytes per voxel.
// The march reads both flavours with the same instructions: only the address tables (vr_raymarch_body.inc) and the builder differ.
constexpr uint32_t kRun7Cells = 7, kRun7Len = 8, kRun7Bytes = kRun7Len * 4, kRun7BrickBytes = 64 * kRun7Bytes;
__host__ __device__ constexpr uint32_t run7_bricks(uint32_t n) { return (n + kRun7Cells - 1u) / kRun7Cells; }
inline uint64_t run7_copy_bytes(uint32_t dim_x, uint32_t dim_other, uint32_t dim_run) {       // the same 16 bytes of tail slack
	return (uint64_t) ((dim_x + 7) / 8) * ((dim_other + 7) / 8) * run7_bricks(dim_run) * kRun7BrickBytes + 16;
}
enum : uint32_t { kLaneRows = 0, kLaneColumns = 1, kLaneBlocks = 2 };
constexpr uint32_t kBrickEdge = 8, kBrickPitch = 512;

// Where each coordinate bit lands inside the 9-bit element offset of a brick: positions of x0 x1 x2, y0 y1 y2, z0 z1 z2.
//  * 1-byte voxels (4-byte elements): a0 b0 | a1 b1 | c0 | a2 b2 | c1 c2 for a "chunk plane" (a,b) — every aligned 16-byte
//    chunk (the unit the vector memory pipeline serves a lane quad from) is a 2x2 (a,b) block of elements, every 64 bytes a
//    4x4 block, every 128-byte line a 4x4x2 block.  Up to three copies exist, one per chunk plane (x,y) / (x,z) / (y,z);
//    the host picks the plane perpendicular to the view's dominant axis (vr_hip_api.cpp), NEAREST always reads (x,y);
//  * 2-byte voxels (8-byte elements, served at one lane quad per step whatever the order): plain Z-order with z in the
//    lowest, y in the middle and x in the top slot — measured 10 % faster than the order above on 1024^3 u16.
// All measured against the alternatives with scripts/gpu_variants.sh / gpu_planes.sh.
enum : uint32_t { kPlaneXY = 0, kPlaneXZ = 1, kPlaneYZ = 2, kPlanes = 3 };
// the brick copies a context may hold (bit i of vr_hip_prepare's mask / vr_volume_info::copies = copy i): quad bricks per chunk
// plane, run bricks along z / y, voxel bricks
enum : uint32_t { kCopyQuadXY = 0, kCopyQuadXZ = 1, kCopyQuadYZ = 2, kCopyRunZ = 3, kCopyRunY = 4, kCopyVoxel = 5, kCopyOct = 6,
                  kCopyColX = 7, kCopyColY = 8, kCopyColZ = 9,        // column windows along x / y / z (kLayoutColumn), quad elements: TRILINEAR
                  kCopyColVoxX = 10, kCopyColVoxY = 11, kCopyColVoxZ = 12,      // ... of plain voxels: NEAREST
                  kCopyKinds = 13 };
static_assert(kCopyKinds == VR_COPY_KINDS, "include/vr_hip.h VR_COPY_KINDS");
// ... and behind the kinds vr_volume_info counts (its build_ms array keeps VR_COPY_KINDS slots): the aligned run bricks along z / y
// (above).  Not in VR_COPY_ALL nor in the policy's default set: built on first use by a full-march frame that reads run bricks, or by
// vr_hip_prepare when their bit is named; reported by vr_hip_run_aligned_info.
enum : uint32_t { kCopyRun7Z = kCopyKinds, kCopyRun7Y = kCopyKinds + 1, kCopySlots = kCopyKinds + 2 };
static_assert((1u << kCopyRun7Z) == VR_COPY_RUN7_Z && (1u << kCopyRun7Y) == VR_COPY_RUN7_Y, "include/vr_hip.h VR_COPY_RUN7_*");
// column windows (kLayoutColumn): lateral axes (u, v) of march axis m are the two other axes in increasing order
// A lateral block is kColEdge x kColEdge cell columns: its windows are kColBlockBytes each and follow each other along m.  4 x 4 columns
// = what one wave's 8 x 8 pixels cover at the reference's zoom, 256 bytes per window.  Measured against 8 x 8 columns (1 KiB per window
// of a block, -DVR_COL_EDGE_LOG2=3; full march, the three axis-aligned poses): 1.79 / 1.84 / 2.30 ms against 1.82 / 1.88 / 2.59 ms.
#ifndef VR_COL_EDGE_LOG2
#define VR_COL_EDGE_LOG2 2
#endif
constexpr uint32_t kColEdgeLog2 = VR_COL_EDGE_LOG2, kColEdge = 1u << kColEdgeLog2, kColEdgeMask = kColEdge - 1u;
constexpr uint32_t kColCells = 3, kColWindowBytes = 16, kColRowBytes = kColEdge * kColWindowBytes, kColBlockBytes = kColEdge * kColRowBytes;       // cells per window; edge x edge columns x 16 bytes
// NEAREST reads ONE voxel per sample: its column windows hold 16 consecutive voxels of the column (cells 16w .. 16w+15, the index
// clamped at Nm - 1) in the same block / window geometry — one 16-byte gather and one transparency test per SIXTEEN samples, 1 byte per voxel.
constexpr uint32_t kColVoxCells = 16;
__host__ __device__ constexpr uint32_t col_blocks(uint32_t n) { return (n + kColEdgeMask) >> kColEdgeLog2; }
__host__ __device__ constexpr uint32_t col_axis_u(uint32_t m) { return m == 0u ? 1u : 0u; }
__host__ __device__ constexpr uint32_t col_axis_v(uint32_t m) { return m == 2u ? 1u : 2u; }
__host__ __device__ inline uint32_t col_windows(uint32_t nm, uint32_t cells = kColCells) { return (nm + cells - 1u) / cells; }
// Where cell column (u, v) lies in a window copy — the one statement of the layout for everything that reads it (column_build_kernel
// writes in copy order and never forms a column's address).  The lateral blocks follow each other along u, then v, each a run of
// `windows` windows of kColBlockBytes along m; inside every window of its block the column's 16 bytes sit at row v, place u.
__host__ __device__ constexpr uint32_t col_lateral_block(uint32_t u, uint32_t v, uint32_t blocks_u) { return (v >> kColEdgeLog2) * blocks_u + (u >> kColEdgeLog2); }
__host__ __device__ constexpr uint32_t col_in_block(uint32_t u, uint32_t v) { return (v & kColEdgeMask) * kColRowBytes + (u & kColEdgeMask) * kColWindowBytes; }
// byte offset of the column's first window: 32-bit (copies below 4 GiB), and 64-bit from the byte strides between lateral blocks
// (stride_u = windows * kColBlockBytes, stride_v = blocks_u * stride_u), one axis at a time (in_block: kColWindowBytes along u, kColRowBytes along v) or both
__host__ __device__ constexpr uint32_t col_lateral_offset(uint32_t u, uint32_t v, uint32_t blocks_u, uint32_t windows) {
	return col_lateral_block(u, v, blocks_u) * windows * kColBlockBytes + col_in_block(u, v);
}
__host__ __device__ constexpr uint64_t col_axis_offset64(uint32_t c, uint64_t block_stride, uint32_t in_block) { return (uint64_t) (c >> kColEdgeLog2) * block_stride + (c & kColEdgeMask) * in_block; }
__host__ __device__ constexpr uint64_t col_lateral_offset64(uint32_t u, uint32_t v, uint64_t stride_u, uint64_t stride_v) {
	return col_axis_offset64(u, stride_u, kColWindowBytes) + col_axis_offset64(v, stride_v, kColRowBytes);
}
// The march prefetches windows past a ray's exit and addresses them by a running pointer without clamping the window index: inside
// the copy that reads a neighbouring block's windows (never used: those samples lie outside every segment), at its two ends it reads
// this much zeroed padding (64 windows).  The kernel bounds its window count by the windows left in march direction + kColSlots + 2 (colmarch_kernel).
constexpr uint32_t kColPadBytes = 64u * kColBlockBytes;
inline uint64_t col_copy_bytes(const uint32_t dim[3], uint32_t m, bool voxels = false) {      // without the padding
	return (uint64_t) col_blocks(dim[col_axis_u(m)]) * col_blocks(dim[col_axis_v(m)]) * col_windows(dim[m], voxels ? kColVoxCells : kColCells) * kColBlockBytes;
}
// bit position of coordinate bit k (0..2) of axis (0 = x, 1 = y, 2 = z)
__host__ __device__ inline uint32_t brick_bit(uint32_t bytes_per_voxel, uint32_t plane, uint32_t axis, uint32_t k) {
	constexpr uint8_t table[4][9] = {
		{ 0, 2, 5, 1, 3, 6, 4, 7, 8 },      // chunk plane (x,y)
		{ 0, 2, 5, 4, 7, 8, 1, 3, 6 },      // chunk plane (x,z)
		{ 4, 7, 8, 0, 2, 5, 1, 3, 6 },      // chunk plane (y,z)
		{ 2, 5, 8, 1, 4, 7, 0, 3, 6 },      // 2-byte voxels: Z-order
	};
	return table[bytes_per_voxel == 2 ? 3u : plane][3 * axis + k];
}
// spread the three low bits of a coordinate to their positions / collect them again
__host__ __device__ inline uint32_t brick_spread(uint32_t bpv, uint32_t plane, uint32_t axis, uint32_t v) {
	return ((v & 1u) << brick_bit(bpv, plane, axis, 0)) | (((v >> 1) & 1u) << brick_bit(bpv, plane, axis, 1)) | (((v >> 2) & 1u) << brick_bit(bpv, plane, axis, 2));
}
__host__ __device__ inline uint32_t brick_collect(uint32_t bpv, uint32_t plane, uint32_t axis, uint32_t local) {
	return ((local >> brick_bit(bpv, plane, axis, 0)) & 1u) | (((local >> brick_bit(bpv, plane, axis, 1)) & 1u) << 1) | (((local >> brick_bit(bpv, plane, axis, 2)) & 1u) << 2);
}

// Volume resident in HBM: the reference's linear layout (x fastest, then y, then z — ModelBase.h:18-22) followed by
// kTailSlack zeroed elements, so the +1 neighbours of a trilinear fetch at the upper faces (weight exactly 0) stay
// inside the allocation.
inline uint64_t volume_tail_slack(uint32_t dim_x, uint32_t dim_y) { return (uint64_t) dim_x * dim_y + dim_x + 2; }

// linear -> quad-brick copy
hipError_t launch_brickify(const void *linear, void *bricked, uint32_t bytes_per_voxel, uint32_t plane, uint32_t dim_x, uint32_t dim_y,
                           uint32_t dim_z, hipStream_t stream);
// linear -> voxel bricks (NEAREST): element (x,y,z) = the voxel, brick order of the (x,y) quad copy
hipError_t launch_brickify_voxel(const void *linear, void *voxel_bricks, uint32_t bytes_per_voxel, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z,
                                 hipStream_t stream);
// linear -> oct bricks (2-byte voxels): element = the 2x2x2 neighbourhood, 16 bytes
hipError_t launch_brickify_oct(const void *linear, void *oct_bricks, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, hipStream_t stream);
// linear -> run bricks (1-byte voxels)
hipError_t launch_brickify_run(const void *linear, void *run_copy, uint32_t run_layout /* kLayoutRun | kLayoutRunY */, bool aligned /* 32-byte runs of seven cells */,
                               uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, hipStream_t stream);
// linear -> column windows along axis m (1-byte voxels)
hipError_t launch_build_column(const void *linear, void *col_copy, uint32_t axis, bool voxels /* NEAREST windows */, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, hipStream_t stream);
// number of quad elements (each 4 * bytes_per_voxel bytes)
inline uint64_t bricked_elems(uint32_t dim_x, uint32_t dim_y, uint32_t dim_z) {
	return (uint64_t) ((dim_x + kBrickEdge - 1) / kBrickEdge) * ((dim_y + kBrickEdge - 1) / kBrickEdge) *
	       ((dim_z + kBrickEdge - 1) / kBrickEdge) * kBrickPitch;
}

// `linear` is the reference's array; `bricked` the brick copy RayKernelArgs::layout names (quad bricks of plane
// brick_plane, or the run bricks) or NULL (VR_LAYOUT_LINEAR).
typedef hipError_t CompositeLauncher(const RayKernelArgs &a, const void *linear, const void *bricked, uint32_t bytes_per_voxel,
                                     const float *tf_premult /* 128 x float4 */, const uint32_t *esl_bits /* 1024 */,
                                     void *out_rgba, TileSchedule sched, hipStream_t stream);
CompositeLauncher launch_raymarch;
// The feature frames launch_raymarch hands over, one launcher per kernel unit (the kernels of each are declared there through
// vr_composite_family.inc); each refuses a frame that is not its own with hipErrorInvalidValue:
//  * vr_shadow.hip: the shadowed frame (a.shadow_on; vr_hip_set_shadow), raymarch_shadowed;
//  * vr_light.hip: the gradient-lit frame (a.light_on; vr_hip_set_lighting, section 4.8), composite_lit;
//  * vr_slab.hip: the pre-integrated frame (a.slab_on; vr_hip_set_preintegration, section 4.10), composite_slab or, with a.light_on,
//    composite_slab_lit.  tf_premult: the 128 entries and K behind them, here and in vr_backdrop_slab.hip;
//  * vr_backdrop.hip (without a.slab_on) and vr_backdrop_slab.hip (with it): the backdrop frame (a.backdrop_on; vr_hip_render_backdrop,
//    section 4.11), composite_backdrop / composite_backdrop_slab or, with a.light_on, their _lit kernels.  out_rgba may be the colour layer.
CompositeLauncher launch_raymarch_shadowed, launch_composite_lit, launch_composite_slab, launch_composite_backdrop, launch_composite_backdrop_slab;
// the column kernels' frame (a.layout kLayoutColumn / kLayoutVoxCol, `copy` = those column windows; a clipped frame is
// hipErrorInvalidValue): launch_raymarch hands it over, vr_kernels.hip launches it
hipError_t launch_colmarch(const RayKernelArgs &a, const void *copy, const float *tf_premult, void *out_rgba, hipStream_t stream);

// what launch_raymarch will do with these arguments: whether the variant reads the LINEAR array (refused once that was released),
// and its grid of workgroup tiles (32x16 pixels, 32x32 for the 64-bit address tables)
struct RaymarchPlan { bool reads_linear; uint32_t tiles_x, tiles_y; uint32_t tile_h = 16; /* rows of a workgroup tile (32 pixels wide) */ };
RaymarchPlan plan_raymarch(const RayKernelArgs &a, bool have_bricked, uint32_t bytes_per_voxel);
// cost[ntiles] (recorded by a frame) -> order[ntiles] for the next frame with the same parameters; clears cost
hipError_t launch_tile_order(uint32_t *cost, uint32_t *order, uint32_t ntiles, hipStream_t stream);
// predicted cost[ntiles] for a frame that leaps and has no recording yet (a.tiles_x / tiles_y / phase filled in; tile_h = rows of a workgroup tile)
hipError_t launch_tile_estimate(const RayKernelArgs &a, uint32_t tile_h, const uint32_t *esl, uint32_t *cost, uint32_t ntiles, hipStream_t stream);
// kLayoutRunDual: choice[t] = t | (cost_y[t] < cost_z[t] ? kTileAltBit : 0); both costs NULL = alternating tiles (testing)
hipError_t launch_tile_choice(const uint32_t *cost_z, const uint32_t *cost_y, uint32_t *choice, uint32_t ntiles, hipStream_t stream);

hipError_t launch_minmax(const void *volume, uint32_t bytes_per_voxel, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z,
                         uint32_t esl_block_dims, uint8_t *minmax_dev /* 32768 x {min,max} */, hipStream_t stream);

// ---- maximum-intensity projection (include/vr_hip.h vr_hip_render_mip) ----
// The bounds a MIP frame skips fetches by, derived from the min/max scan: kMipBoundEntries bytes for NEAREST (entry = the block's
// maximum), the same again for TRILINEAR (entry = the maximum over the 3x3x3 neighbouring blocks: a sample's cell may lie one voxel
// outside its block on each side), then one 32-bit word, the volume's maximum.  Entry index z*1024 + y*32 + x like the scan; 2-byte
// volumes hold the HIGH byte everywhere (the kernel pads it with 0xff: rounding a bound up only loses skips).  The probe build
// (`make EXTRA=-DVR_MIP_STATS`, scripts/mip_probe.py; not the product) keeps two 64-bit counters behind them, at kMipStatsAt: samples
// of the frames that skipped, and fetches they issued.
constexpr uint32_t kMipBoundEntries = VR_ESL_VOLUME_DIMS * VR_ESL_VOLUME_DIMS * VR_ESL_VOLUME_DIMS;
constexpr uint32_t kMipStatsAt = 2u * kMipBoundEntries + 16u, kMipBoundBytes = kMipStatsAt + 16u;
hipError_t launch_mip_bounds(const uint8_t *minmax_dev /* launch_minmax */, uint8_t *bounds_dev /* kMipBoundBytes */, hipStream_t stream);
// One MIP frame.  `a` as for launch_raymarch with layout one of kLayoutLinear / kLayoutBricked / kLayoutVoxel / kLayoutOct (what
// plan_raymarch answers for `a` holds for this launch too: same selector, same tile grid); a.p.esl != 0 = skip and stop by `bounds`
// (then not NULL) with the block grid of a.esl_div_*, which the caller takes from the VOLUME (vr_hip_volume_minmax), not from a.p.
hipError_t launch_mip(const RayKernelArgs &a, const void *linear, const void *bricked, uint32_t bytes_per_voxel, const float *tf_premult,
                      const uint8_t *bounds, void *out_rgba, hipStream_t stream);

// ---- shaded isosurface with depth (include/vr_hip.h vr_hip_render_iso) ----
// One isosurface frame.  `a`, `linear`, `bricked` and `bounds` as for launch_mip, a.p.sampling TRILINEAR or TRILINEAR_Q8 (anything else, or a
// layout a MIP frame of those samplings never takes, is hipErrorInvalidValue); a.p.esl != 0 = skip the fetch of samples whose widened
// TRILINEAR bound (the second half of `bounds`) is below `level`.  out_depth (out_width * out_rows floats, laid out like out_rgba) may be NULL.
hipError_t launch_iso(const RayKernelArgs &a, const void *linear, const void *bricked, uint32_t bytes_per_voxel, const float *tf_premult,
                      const uint8_t *bounds, float level, uint32_t refine, void *out_rgba, void *out_depth, hipStream_t stream);

// ---- section frames (include/vr_hip.h vr_hip_render_section) ----
// The section of one frame, a kernel argument of its own behind the ones a MIP frame takes: vr_section with the window prepared.
struct SectionArgs {
	float    plane[4];                 // n.x, n.y, n.z, d
	float    half_width;               // h (0 for VR_SECTION_POINT)
	uint32_t mode;                     // vr_section_mode
	uint32_t windowed;                 // 1: grey window, 0: colour by the transfer function
	float    window_lo, window_inv;    // lo and 1.0f / (hi - lo), the division done once on the host
};
// One section frame.  `a`, `linear` and `bricked` as for launch_iso (the same rows: a.p.sampling TRILINEAR or TRILINEAR_Q8), the clip words of
// `a` filled (the identity clip when none is set: the kernel always runs clip_segment); a.p.esl is not looked at.  out_depth may be NULL.
hipError_t launch_section(const RayKernelArgs &a, const SectionArgs &section, const void *linear, const void *bricked, uint32_t bytes_per_voxel,
                          const float *tf_premult, void *out_rgba, void *out_depth, hipStream_t stream);

// ---- depth frames of the composite and picking (include/vr_hip.h vr_hip_render_depth) ----
// The depth of one frame, a kernel argument of its own behind the ones a composite frame takes.
struct DepthArgs {
	float    opacity;                  // FIRST: the accumulated alpha a surface lies at
	uint32_t mode;                     // vr_depth_mode
	uint32_t slab;                     // 1: slab classification (vr_hip_set_preintegration), 0: the filtered lookup
	uint32_t want_alpha;               // 0: no alpha buffer is asked for — a FIRST ray may stop at its surface
};
// One depth frame.  `a`, `linear` and `bricked` as for launch_section (the same rows), the clip words of `a` filled; a.p.esl != 0 = leap with
// esl_bits (1024 words) and the block grid of a.esl_div_*, the caller's params'; a.skip_mask / skip_cmp / tf_zero_below as launch_raymarch takes
// them.  tf_premult: the 128 entries and K behind them.  out_value and out_alpha may be NULL.
hipError_t launch_depth(const RayKernelArgs &a, const DepthArgs &depth, const void *linear, const void *bricked, uint32_t bytes_per_voxel,
                        const float *tf_premult, const uint32_t *esl_bits, void *out_depth, void *out_value, void *out_alpha, hipStream_t stream);
// The pick's finishing kernel: query i's pixel (xy[2i], xy[2i+1]) of the view of a.p, its depth / value / alpha at element i of the three
// arrays -> out[i] (vr_pick), position and voxel index formed on the device from pixel_ray of that pixel.
hipError_t launch_pick_finish(const RayKernelArgs &a, uint32_t n, const uint32_t *xy, const float *depth, const float *value, const float *alpha,
                              vr_pick *out, hipStream_t stream);

// ---- labelled composite frames (include/vr_hip.h vr_hip_render_labelled) ----
// The labels of one frame, a kernel argument of its own behind the ones a composite frame takes.
struct LabelArgs {
	uint64_t labels;                   // the label array the frame reads: one byte per voxel
	uint32_t bricked;                  // 1: `labels` is in the 1-byte voxel-brick order of chunk plane (x,y) (launch_brickify_voxel) and the frame
	                                   // reads the (x,y) quad copy of 1-byte voxels behind address tables, whose entries address it too; 0: linear
	uint32_t reserved;
};
// One labelled frame.  `a`, `linear` and `bricked` as for launch_depth (the same rows), the clip words of `a` filled, the lighting and shadow
// words as launch_raymarch takes them (a.light_on, a.shadow_on: wave-uniform arguments of the one family); a.p.esl, a.esl_div_*,
// a.skip_mask / skip_cmp / tf_zero_below likewise.  labels_linear: the label array in the volume's linear order (+ its tail slack);
// labels_xy_bricks: its 1-byte voxel-brick copy, or NULL — read instead where the row the frame runs addresses the (x,y) quad copy of 1-byte
// voxels through tables (the launcher decides: the selector is its own).  table: VR_LABEL_COUNT entries of 5 floats (vr_label_entry) on the device.
hipError_t launch_labelled(const RayKernelArgs &a, const void *labels_linear, const void *labels_xy_bricks, const void *linear, const void *bricked,
                           uint32_t bytes_per_voxel, const float *tf_premult, const uint32_t *esl_bits, const float *table, void *out_rgba, hipStream_t stream);

// ---- 2D transfer-function frames (include/vr_hip.h vr_hip_render_tf2d) ----
// The second axis of one frame, a kernel argument of its own behind the ones a composite frame takes.
struct Tf2dArgs {
	float    g_scale;                  // row coordinate = fmed3(g * g_scale, 0, top)
	float    top;                      // (float) (rows - 1)
	uint32_t last;                     // rows - 2: the highest lower row
	uint32_t rows;                     // 2..VR_TF2D_ROWS_MAX: rows * VR_TF_SIZE entries of the table are staged
	uint32_t g_dependent[4];           // bit i: some row differs from row 0 at entry i or at min(i + 1, 127)
};
// One tf2d frame.  `a`, `linear` and `bricked` as for launch_labelled (the same rows), the clip, lighting and shadow words likewise; a.p.esl,
// a.esl_div_* as launch_depth takes them; a.skip_mask / skip_cmp / tf_zero_below are the ENVELOPE's (the per-channel maximum over the rows).
// table: rows * VR_TF_SIZE float4 on the device, row-major; esl_bits: the table's own 1024 words.
hipError_t launch_tf2d(const RayKernelArgs &a, const Tf2dArgs &d, const void *linear, const void *bricked, uint32_t bytes_per_voxel,
                       const float *table, const uint32_t *esl_bits, void *out_rgba, hipStream_t stream);
// The histogram over (value bin, gradient-magnitude row) of the linear array: hist_dev[g_bins * 256] is zeroed and filled on `stream`.
// `bc` (bounds-checked build alone): volume_args with bc_base / bc_bytes / bc_fault armed for the linear array.
hipError_t launch_gradient_histogram(const void *volume, uint32_t bytes_per_voxel, const uint32_t dims[3], uint32_t g_bins, float g_scale,
                                     unsigned long long *hist_dev, const RayKernelArgs *bc, hipStream_t stream);

// ---- fused composite frames (include/vr_hip.h vr_hip_render_fused) ----
// The second field of one frame, a kernel argument of its own behind the ones a composite frame takes.
struct FusedArgs {
	uint64_t vol_b;                    // field B in the order of the array the row reads of field A (filled by launch_fused)
	float    weight_a, weight_b;       // vr_fusion
	uint32_t mode;                     // VR_FUSE_SUM / VR_FUSE_OVER, wave-uniform
	uint32_t skip_mask_b, skip_cmp_b;  // the corner test of B's transfer function (RayKernelArgs::skip_mask / skip_cmp are A's)
	float    tf_zero_below_b;          // ... and its leading all-zero entries
};
// One fused frame.  `a`, `linear` and `bricked` as for launch_labelled (the same rows), the clip, lighting and shadow words likewise; a.p.esl,
// a.esl_div_* as launch_depth takes them; a.skip_mask / skip_cmp / tf_zero_below are field A's function's.  second_linear: B's linear array
// (+ the tail slack of the volume's); second_bricked: B's copy in the layout and chunk plane of `bricked`, NULL exactly where `bricked` is.
// esl_bits: the fused frame's own 1024 words.  fusion.vol_b is the launcher's to fill.
hipError_t launch_fused(const RayKernelArgs &a, const FusedArgs &fusion, const void *linear, const void *bricked, const void *second_linear,
                        const void *second_bricked, uint32_t bytes_per_voxel, const float *tf_premult, const uint32_t *esl_bits,
                        const float *second_tf_premult, void *out_rgba, hipStream_t stream);

// ---- light-source shadows (include/vr_hip.h vr_hip_set_shadow) ----
// What shadow_build_kernel marches with, besides the volume geometry of RayKernelArgs: one lane per node of the S^3 light grid.
struct ShadowBuildArgs {
	float    light[3];
	uint32_t dims;                     // S
	float    node_scale;               // 2.0f / (float) (S - 1): node position = fma((float) i, node_scale, -1.0f)
	float    step, cutoff;
	uint32_t q8;                       // 1: VR_SAMPLE_TRILINEAR_Q8 weights (volume and transfer function)
	uint32_t max_steps;                // ceil(2 sqrt(3) / step) + 2: the explicit bound of the march, never binding
	uint32_t clip_on;                  // 1: the light ray's segment is narrowed by the clip words of RayKernelArgs (clip_segment)
};
// Builds q[S^3] (x fastest) on `stream`.  `a`: volume_args with layout one of kLayoutLinear / kLayoutBricked (plane (x,y)) / kLayoutOct and
// a.p.sampling TRILINEAR — the copy a TRILINEAR MIP frame along z reads; the selector of launch_raymarch picks the addressing path.
hipError_t launch_shadow_build(const RayKernelArgs &a, const ShadowBuildArgs &s, const void *linear, const void *bricked, uint32_t bytes_per_voxel,
                               const float *tf_premult, uint8_t *q_out, hipStream_t stream);

hipError_t launch_histogram(const void *volume, uint32_t bytes_per_voxel, uint64_t voxels,
                            unsigned long long *hist256_dev, hipStream_t stream);

hipError_t launch_generate(void *volume, uint32_t kind, uint32_t n, uint32_t seed, uint32_t bytes_per_voxel,
                           hipStream_t stream);

}  // namespace vr
