// vr_hip_api.cpp — the C ABI of include/vr_hip.h: one opaque context per GPU that owns the device copies of the
// volume / transfer function / ESL bit-volume / framebuffer and launches the gfx950 kernels of the units behind vr_device.h.
//
// It replaces the device management the reference spreads over GPURenderer1.cu:17-28,65-112, GPURenderer23.cu:55-81
// and GPURenderer4.cu:89-153 (static globals, cudaMalloc/cudaMemcpy per set_*, cuda_safe_call -> exit).  Differences
// by design: no globals, no exit(), errors are return codes + vr_hip_last_error(); the per-frame parameter block is
// the kernel argument itself (no cudaMemcpyToSymbol per frame, GPURenderer23.cu:65,77); the frame clear is fused into
// the kernel (no cudaMemset per frame, GPURenderer1.cu:107).  There is no CPU fallback.
#include "vr_device.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace vr;

#ifndef VR_ORDER_ALWAYS
#define VR_ORDER_ALWAYS 0      // 1: the measured-cost tile order also for the full march (A/B: TRILINEAR +2 %, NEAREST -2 %)
#endif

namespace {

constexpr int kEventRing = 256;

struct EventPair { hipEvent_t start = nullptr, stop = nullptr; bool pending = false; };

}  // namespace

struct vr_ctx {
	int device = -1;
	hipStream_t stream = nullptr;           // context-owned stream for the synchronous entry points
	hipStream_t stream_first = nullptr;     // vr_hip_render: the first row slice of a frame runs here, AHEAD of the rest (highest stream priority)
	// window
	uint32_t win_w = 0, win_h = 0;
	void *fb = nullptr; size_t fb_bytes = 0;
	// transfer function + ESL
	float *tf = nullptr; uint32_t *esl = nullptr; bool tf_set = false;
	float tf_zero_below = -1.0f;            // leading all-zero entries of the resident TF (exact transparent-sample shortcut)
	// volume
	void *vol = nullptr; uint64_t vol_elems = 0; uint32_t dim[3] = { 0, 0, 0 }; uint32_t bpv = 0;
	// Brick copies of the resident volume (vr_device.h), built ON FIRST USE by the frame that wants them (or ahead of time by
	// vr_hip_prepare): a NEAREST-only session never pays for the quad / run copies, a session that only looks along z never
	// builds the (x,z) / (y,z) planes.  copy[kCopyQuadXY..YZ] = quad bricks per chunk plane, kCopyRunZ / kCopyRunY = run bricks,
	// kCopyVoxel = voxel bricks (what NEAREST reads), kCopyOct = oct bricks (what TRILINEAR reads for 2-byte voxels).  copy_failed: a build was refused (HBM guard / allocation) — not retried
	// until the next set_volume, so a frame never stalls twice on the same refusal.
	void *copy[kCopySlots] = {};            // kCopyColX..Z = column windows along x / y / z (orthogonal full-march frames along that axis)
	float copy_build_ms[kCopySlots] = {};   // kCopyRun7Z / Y (behind the kCopyKinds kinds vr_volume_info counts) = the aligned run bricks: full-march frames that read run bricks
	bool copy_failed[kCopySlots] = {};
	uint32_t run_flavour = 0;               // vr_hip_set_run_flavour: 0 = automatic, 1 = nine-element runs, 2 = seven-cell aligned runs (full-march frames)
	uint32_t last_run_flavour = 0;          // vr_hip_run_aligned_info: what the last composite frame read (0 no run bricks, 1 nine-element, 2 aligned)
	int32_t column_force = 0;               // vr_hip_set_brick_plane: 0 = per view (views along a volume axis), 1 (plane 8) = every orthogonal full-march frame, -1 (plane 9) = never
	uint32_t column_copy = 0;               // vr_hip_set_column_copy: 0 = TRILINEAR column frames read the voxel windows where a wave's columns fit (lit frames shade from the
	                                        // quad-element windows), 1 = the quad-element windows, 2 = as 0, shading by byte loads from the voxel windows (no second copy)
	float upload_ms = 0;                    // host -> HBM copy (or generation) of the linear array in the last set_volume
	int32_t brick_plane_force = -1;         // -1 = per view (plane perpendicular to the dominant view axis; run bricks for oblique views),
	                                        // 0..2 = that chunk plane, 3 = the run bricks (testing)
	uint32_t layout = VR_LAYOUT_BRICKED;
	uint32_t force_wide = 0;
	uint32_t force_clamp_fetch = 0;              // testing aid (vr_hip_set_wide_addressing bit 2)
	int32_t  tile_lane_map = -1;                 // -1 = choose per frame (choose_tile_mapping), else forced
	uint32_t tile_phase_x = 0, tile_phase_y = 0;
	// the last few automatic tile mappings (lane order, tile phase), keyed by the frame parameters and the volume size (a benchmark
	// cycles 8 views).  cost / order / dual_state / order_ready / order_stream serve only the MEASURED run-copy choice
	// (vr_hip_set_brick_plane(6), the validator of the analytic rule: frames 0 / 1 of a parameter set run on the copy along z / y,
	// frames 2 / 3 do so again and record their tile costs, the choice kernel behind frame 3 fills order[], frames 4.. read it).
	struct MapEntry { vr_params p; uint32_t dim[3]; uint32_t lane_map, phase_x, phase_y, straddle_permille;
	                  uint32_t *cost = nullptr, *order = nullptr; uint32_t capacity = 0, order_tiles = 0;
	                  uint32_t dual_state = 0;
	                  hipEvent_t order_ready = nullptr; hipStream_t order_stream = nullptr; };
	MapEntry map_cache[32]; uint32_t map_cached = 0, map_next = 0;      // (8 benchmark views x the two row slices of vr_hip_render, and the whole frames beside them)
	// Measured-cost launch orders (vr_schedule.hip tile_order_kernel), keyed by what the cost of a tile DEPENDS on — sampling mode,
	// leaping / termination on or off, projection, the view's major axis, the band partition, the tile grid and the copy read — not by
	// the byte image of the parameters: a camera that moves keeps its entry, every frame launches its tiles in the order the most recent
	// FINISHED recording gives and records its own costs for the next one; a frame repeated with identical parameters stops recording
	// after two (the first may have run on cold caches).  Three slots per entry so that frames in flight on several streams never
	// share a buffer that is being rewritten: a slot is recycled only once every frame that read or recorded it is known to have
	// finished (the event ring below) and its order kernel has run (`ready`) — ADVICE r3: no buffer of a frame in flight is touched.
	struct SchedSlot { uint32_t *cost = nullptr, *order = nullptr; uint32_t capacity = 0, ntiles = 0; hipEvent_t ready = nullptr; hipStream_t stream = nullptr;
	                   uint64_t last_seq = 0, issue_seq = 0; bool valid = false; };
	struct OrderKey { int32_t direction_q[3]; uint32_t sampling, esl, ert, perspective, major_axis, layout, view_w, view_h, x0, out_width, out_rows, band_rows, band_stride, band_first,
	                  dim[3], tiles_x, tiles_y; };
	struct OrderEntry { OrderKey key; bool used = false; SchedSlot slot[3]; vr_params last; bool has_last = false; uint32_t repeats = 0; uint64_t lru = 0; };
	OrderEntry order_cache[32];
	uint64_t seq_next = 1, completed_seq = 0;      // frames launched so far + 1; every frame <= completed_seq is known to have finished
	uint64_t ring_seq[kEventRing] = {};            // the frame whose events sit in ring entry i
	uint32_t tile_scheduling = 1;           // vr_hip_set_tile_scheduling: 0 = tile = workgroup id, 1 = measured-cost order, 2 = cost map
	vr_launch_info last_launch = {};        // vr_hip_last_launch
	uint32_t *cost_map = nullptr;           // mode 2: what every tile of the LAST frame cost (vr_hip_read_tile_costs)
	size_t cost_map_bytes = 0; uint32_t cost_map_tiles_x = 0, cost_map_tiles_y = 0;
	bool oct_always = false;                // vr_hip_set_brick_plane(5): 2-byte voxels read the oct bricks for every view (testing)
	// feeders scratch
	uint8_t *minmax = nullptr; unsigned long long *hist = nullptr;
	// maximum-intensity projection: the bounds its frames skip fetches by (vr_device.h kMipBoundBytes), built from the min/max scan by the
	// first frame that skips, kept until the volume changes; and the tile mappings chosen for its last few views
	uint8_t *mip_bounds = nullptr; bool mip_bounds_ready = false;
	struct MipMap { vr_params p; uint32_t dim[3], layout, brick_plane, lane_map, phase_x, phase_y, straddle_permille; };
	MipMap mip_map[16]; uint32_t mip_mapped = 0, mip_map_next = 0;
	// isosurface: the depth buffer of the host entry point (vr_hip_render_iso), one float per pixel of the window, allocated on first use
	float *iso_depth = nullptr; size_t iso_depth_bytes = 0;
	// clip region (vr_hip_set_clip): narrows the segment of every ray of every later frame; such frames run the *_clipped kernels
	bool clip_on = false; vr_clip clip = {};
	// light-source shadows (vr_hip_set_shadow): the S^3 bytes q of the light grid, built on the context's stream by the first composite frame
	// or download that finds them missing or stale (shadow_ready false: a changed shadow, volume, transfer function or clip)
	bool shadow_on = false; vr_shadow shadow = {};
	uint8_t *shadow_q = nullptr; uint64_t shadow_q_bytes = 0; bool shadow_ready = false;
	uint64_t shadow_builds = 0; float shadow_build_ms = 0;
	// gradient lighting (vr_hip_set_lighting): composite frames run the composite_lit kernels; lit_frames counts them (vr_hip_lighting_frames)
	bool lighting_on = false; vr_lighting lighting = {};
	uint64_t lit_frames = 0;
	// pre-integrated classification (vr_hip_set_preintegration): composite frames run the composite_slab / composite_slab_lit kernels;
	// preint_frames counts them (vr_hip_preint_frames).  The integral table K lies behind the 128 entries of `tf` on the device.
	bool preint_on = false;
	uint64_t preint_frames = 0;
	// backdrop frames (vr_hip_render_backdrop / vr_hip_render_hybrid): backdrop_frames counts the composite frames on the composite_backdrop*
	// kernels; the hybrid's depth buffer when the caller gives none and the staging of the host entry points' layers, grown on demand
	uint64_t backdrop_frames = 0;
	// section frames (vr_hip_render_section*): the frames launched on the section kernels
	uint64_t section_frames = 0;
	float *hybrid_depth = nullptr; size_t hybrid_depth_bytes = 0;
	void *backdrop_stage = nullptr; size_t backdrop_stage_bytes = 0;
	// depth frames (vr_hip_render_depth*, vr_hip_pick): the frames launched on the depth kernels (a pick counts one per query); the three
	// float buffers of the host entry point, grown on demand; and the pick's buffers, allocated on first use for VR_PICK_MAX queries: the
	// pixels, depth / value / alpha per query, and the answers
	uint64_t depth_frames = 0;
	void *depth_stage = nullptr; size_t depth_stage_bytes = 0;
	void *pick_stage = nullptr; size_t pick_stage_bytes = 0;
	// label volumes (vr_hip_set_labels, vr_hip_set_label_table, vr_hip_render_labelled*): one byte per voxel of the resident volume in the
	// linear order (+ the volume's zeroed tail slack), dropped with the volume; its copy in the 1-byte voxel-brick order of chunk plane (x,y),
	// built by the first frame that reads it (label_bricks_failed: refused, not retried until the labels change); the table, VR_LABEL_COUNT
	// entries of 5 floats on the device, identity until set; the frames launched on the label kernels
	uint8_t *labels = nullptr, *label_bricks = nullptr; bool label_bricks_failed = false;
	float *label_table = nullptr;
	uint64_t labelled_frames = 0;
	// 2D transfer-function frames (vr_hip_set_tf2d, vr_hip_render_tf2d*): the table (VR_TF2D_ROWS_MAX * VR_TF_SIZE float4, the rows given and
	// zeros behind them) and its own ESL words on the device, both NULL until a table is set; what the host derives from the table — the
	// envelope's leading all-zero entries (tf_zero_below of such a frame) and the 128 g-dependence flags —; the frames launched; and the
	// counters of vr_hip_gradient_histogram (VR_GRADIENT_BINS_MAX * 256), allocated on first use
	float *tf2d_table = nullptr; uint32_t *tf2d_esl = nullptr;
	uint32_t tf2d_rows = 0; float tf2d_g_scale = 0.0f, tf2d_zero_below = -1.0f; uint32_t tf2d_g_dependent[4] = { 0, 0, 0, 0 };
	uint64_t tf2d_frames = 0;
	// fused frames (vr_hip_set_second_volume, vr_hip_set_second_transfer_fn, vr_hip_render_fused*): field B in the linear order of the
	// resident volume (+ its tail slack), dropped with it (drop_second); B's copies in the orders a fused frame reads the resident volume in —
	// the three quad copies and the oct copy —, each built by the first frame that reads it (second_copy_failed: refused, not retried until B
	// changes); B's transfer function and the fused frame's own ESL words on the device, which survive a volume change; the frames launched
	void *second = nullptr;
	void *second_copy[4] = { nullptr, nullptr, nullptr, nullptr }; bool second_copy_failed[4] = { false, false, false, false };
	float *second_tf = nullptr; uint32_t *fused_esl = nullptr; float second_zero_below = -1.0f;
	uint64_t fused_frames = 0;
	unsigned long long *gradient_hist = nullptr;
#ifdef VR_BOUNDS_CHECK
	uint32_t *bc_fault = nullptr;           // debug build: first out-of-bounds access of a frame (RayKernelArgs::bc_fault)
#endif
	// timing
	EventPair ring[kEventRing]; int ring_head = 0;
	hipEvent_t aux_start = nullptr, aux_stop = nullptr;
	float last_kernel_ms = 0, last_total_ms = 0; uint64_t launches = 0; double kernel_ms_sum = 0; float kernel_ms_max = 0, total_ms_max = 0;
	std::string err;
};

namespace {

int fail(vr_ctx *c, int code, const char *what, hipError_t e = hipSuccess) {
	if (c) {
		char buf[512];
		if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s (%d)", what, hipGetErrorString(e), (int) e);
		else snprintf(buf, sizeof buf, "%s", what);
		c->err = buf;
	}
	return code;
}

#define VR_TRY(c, expr)                                                                              \
	do {                                                                                             \
		hipError_t e_ = (expr);                                                                      \
		if (e_ != hipSuccess) {                                                                      \
			(void) hipGetLastError();                                                                \
			return fail((c), e_ == hipErrorOutOfMemory ? VR_ERR_ALLOC : VR_ERR_HIP, #expr, e_);      \
		}                                                                                            \
	} while (0)

bool copy_possible(const vr_ctx *c, uint32_t kind);
uint64_t copy_bytes(const vr_ctx *c, uint32_t kind);
hipError_t drain(vr_ctx *c);
const void *copy_for(vr_ctx *c, uint32_t kind);
int grow_buffer(vr_ctx *c, void **buffer, size_t &have, size_t bytes);

uint32_t max_dim_of(const vr_ctx *c) { return std::max(c->dim[0], std::max(c->dim[1], c->dim[2])); }

bool finite3(const float *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// folds one finished event pair into the statistics
void harvest(vr_ctx *c, EventPair &p) {
	if (!p.pending) return;
	float ms = 0;
	if (hipEventSynchronize(p.stop) == hipSuccess && hipEventElapsedTime(&ms, p.start, p.stop) == hipSuccess) {
		c->last_kernel_ms = ms; c->kernel_ms_sum += ms; c->launches++;
		if (ms > c->kernel_ms_max) c->kernel_ms_max = ms;
	}
	p.pending = false;
}

int validate_params(vr_ctx *c, const vr_params *p) {
	if (p == nullptr) return fail(c, VR_ERR_INVALID, "params is NULL");
	const vr_view &v = p->view;
	if (v.width == 0 || v.height == 0 || v.width > 65535u || v.height > 65535u)      // View::dims is ushort2
		return fail(c, VR_ERR_INVALID, "view dims out of range (1..65535)");
	if (!finite3(v.origin) || !finite3(v.direction) || !finite3(v.right_plane) || !finite3(v.up_plane) || !finite3(v.light_pos))
		return fail(c, VR_ERR_INVALID, "view vectors must be finite");
	if (!(p->ray_step >= 1e-6f) || !std::isfinite(p->ray_step))
		return fail(c, VR_ERR_INVALID, "ray_step must be finite and >= 1e-6");
	if (!std::isfinite(p->ray_threshold) || !std::isfinite(p->light_kd))
		return fail(c, VR_ERR_INVALID, "ray_threshold / light_kd must be finite");
	// The per-wave shortcuts for transparent samples skip the `acc.w > threshold` test, which is exact only if that test cannot
	// newly fire at an unchanged acc.w >= 0, i.e. for threshold >= 0 (the reference's setter keeps it in [0.5, 1], RaycasterBase.cpp:31-33)
	if (p->ray_threshold < 0.0f)
		return fail(c, VR_ERR_INVALID, "ray_threshold must be >= 0");
	if (p->esl && (p->esl_block_dims == 0 || p->esl_block_dims > 65535u || !finite3(p->esl_block_size)))   // unsigned short in the reference
		return fail(c, VR_ERR_INVALID, "esl_block_dims must be in 1..65535 and esl_block_size finite when esl is on");
	if (p->sampling != VR_SAMPLE_NEAREST && p->sampling != VR_SAMPLE_TRILINEAR && p->sampling != VR_SAMPLE_TRILINEAR_Q8)
		return fail(c, VR_ERR_INVALID, "unknown sampling mode");
	if (p->out_width == 0 || p->out_rows == 0 || p->out_width > 65535u || p->out_rows > 65535u)
		return fail(c, VR_ERR_INVALID, "out_width / out_rows out of range");
	if (p->band_rows == 0 || p->band_stride == 0 || p->band_first >= p->band_stride)
		return fail(c, VR_ERR_INVALID, "band partition invalid (band_rows > 0, band_first < band_stride)");
	return VR_OK;
}

// Which pixels share a lane quad, and where the tile grid starts — speed only, the image does not depend on it.
// Measured on MI355X (scripts/ubench/tcp_coalesce.hip): the vector memory pipeline handles a wave's
// gather 4 consecutive lanes at a time and runs ~3.5x faster when the 4 addresses share one aligned 16-byte chunk (= the
// 2x2 (x,y) element block of the brick order).  So:
//  * a view along a volume axis puts 2x2-pixel blocks into a quad (kLaneBlocks): at the usual >= 2 pixels per voxel the four
//    samples fall into one or two cells;
//  * any other view keeps 4x1-pixel quads, along the screen axis whose image in the volume stays closest to the x/y plane;
//  * orthogonal views also shift the tile grid by 0..3 pixels so that 4-pixel groups start on even cells (when the pixel
//    pitch is commensurate with the voxel grid — the reference's default zoom — every quad then reads a single chunk).
// Returns, for orthogonal views, how many of the sampled 4-pixel groups still straddle cells under the best phase (per mille);
// 1000 for views whose quads cannot be aligned at all (perspective, or not along an axis).
uint32_t choose_tile_mapping(RayKernelArgs &a) {
	const vr_view &v = a.p.view;
	// voxel-cell coordinate of a position p: TRILINEAR p * N/2 + N/2 - 1/2 (texel space), NEAREST (p + 1) / 2 * N (ModelBase.h:17-23)
	const bool nearest = a.p.sampling == VR_SAMPLE_NEAREST;
	const float half[3] = { a.half_x, a.half_y, a.half_z };
	const float off[3] = { nearest ? a.half_x : a.off_x, nearest ? a.half_y : a.off_y, nearest ? a.half_z : a.off_z };
	float d[3], sx[3], sy[3];
	for (int i = 0; i < 3; i++) { d[i] = v.direction[i] * half[i]; sx[i] = v.right_plane[i] * half[i]; sy[i] = v.up_plane[i] * half[i]; }
	auto norm = [](const float *u) { return std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]); };
	auto major = [](const float *u) { int m = 0; for (int i = 1; i < 3; i++) if (std::fabs(u[i]) > std::fabs(u[m])) m = i; return m; };
	a.lane_map = kLaneRows; a.phase_x = a.phase_y = 0;
	const float dn = norm(d);
	if (!(dn > 0.0f)) return 1000u;
	if (std::fabs(d[major(d)]) > 0.98f * dn) a.lane_map = kLaneBlocks;
	else {
		// 4x1-pixel quads along the screen axis that leaves the chunk plane least: `out` is the axis not in the plane
		// (oblique views always read the (x,y) copy; forced planes are a testing aid)
		const int out = a.brick_plane == kPlaneXY ? 2 : (a.brick_plane == kPlaneXZ ? 1 : 0);
		const float nx = norm(sx), ny = norm(sy);
		if (nx > 0.0f && ny > 0.0f && std::fabs(sy[out]) * nx < std::fabs(sx[out]) * ny) a.lane_map = kLaneColumns;
	}
	if (v.perspective) return 1000u;
	const bool axis_aligned = a.lane_map == kLaneBlocks;
	// orthogonal view: every ray has the same direction; [k_in, k_out] = the central ray's path through the cube
	float k_in = -1e30f, k_out = 1e30f;
	for (int i = 0; i < 3; i++) {
		if (v.direction[i] == 0.0f) continue;
		const float k1 = (-1.0f - v.origin[i]) / v.direction[i], k2 = (1.0f - v.origin[i]) / v.direction[i];
		k_in = std::fmax(k_in, std::fmin(k1, k2)); k_out = std::fmin(k_out, std::fmax(k1, k2));
	}
	if (!(k_in < k_out) || !(k_out < 1e29f)) return 1000u;
	k_in = std::fmax(k_in, 0.0f);
	// Voxel cell of frame pixel (gx, gy) at depth k along volume axis `ax`, with the KERNEL'S OWN fp32 operations (get_ray,
	// then fma(k, A, B) / (pos + 1) * half): pixels of an axis-aligned view at the reference's default zoom sit exactly on
	// cell boundaries, so which neighbour a boundary pixel joins is decided by the last bit — and may change along the ray
	// when the direction carries rounding noise (pose (180,90,0): components of 4e-8), hence several depths are sampled.
	auto cell_of = [&](int ax, long gx, long gy, float k) -> long {
		const float fx = (float) ((int) gx - (int) (v.width / 2u)), fy = (float) ((int) gy - (int) (v.height / 2u));
		float o = v.origin[ax] + v.right_plane[ax] * fx;
		o = o + v.up_plane[ax] * fy;
		float t;
		if (nearest) t = ((o + v.direction[ax] * k) + 1.0f) * half[ax];
		else         t = std::fmaf(k, v.direction[ax] * half[ax], std::fmaf(o, half[ax], off[ax]));
		return (long) std::floor(t);
	};
	// Phase 0..7 of the 8-pixel wave columns / rows along one screen direction.  Primary cost (what the vector memory pipeline
	// charges): 4-pixel groups that leave their aligned cell pair, pixel pairs that straddle two cells.  Secondary: 8-pixel wave
	// edges that are not 4-cell (128-byte line) boundaries — a wave whose 4x4 cells sit inside one line column touches a
	// quarter of the lines, and workgroup footprints that end on line boundaries do not fetch their border lines twice
	// (measured before: 2.0x the compulsory bytes at L2 with 4-pixel alignment only).
	long groups_seen[2] = { 0, 0 }, groups_straddling[2] = { 0, 0 };      // of the winning phase, per screen direction (0 = x, 1 = y)
	auto best_phase = [&](bool horizontal, uint32_t first, uint32_t count, uint32_t other_centre) {
		const float *sdir = horizontal ? sx : sy;
		const int ax = major(sdir);
		const long hi = (long) (2.0f * half[ax]) - 1;
		uint32_t best = 0; long best_cost = -1, best_seen = 0, best_bad = 0;
		for (uint32_t ph = 0; ph < 8; ph++) {
			long cost = 0, seen = 0, bad = 0;
			for (int depth = 0; depth < 4; depth++) {
				const float k = k_in + (k_out - k_in) * (0.125f + 0.25f * (float) depth);
				for (long g0 = -(long) ph; g0 < (long) count; g0 += 8 * 7) {      // every seventh wave column is plenty
					long cell[8]; bool in[8];
					for (int i = 0; i < 8; i++) {
						const long g = (long) first + g0 + i;
						cell[i] = horizontal ? cell_of(ax, g, other_centre, k) : cell_of(ax, other_centre, g, k);
						in[i] = g0 + i >= 0 && g0 + i < (long) count && cell[i] >= 0 && cell[i] <= hi;
					}
					for (int q = 0; q < 8; q += 4) {
						const long before = cost;
						if (in[q] && in[q + 3] && (cell[q] >> 1) != (cell[q + 3] >> 1)) cost += 32;          // the group leaves its aligned cell pair
						if (in[q] && in[q + 1] && cell[q] != cell[q + 1]) cost += 16;                        // a pixel pair straddles two cells
						if (in[q + 2] && in[q + 3] && cell[q + 2] != cell[q + 3]) cost += 16;
						if (in[q] && in[q + 3]) { seen++; if (cost != before) bad++; }
					}
					if (in[0] && in[7] && (cell[0] >> 2) != (cell[7] >> 2)) cost += 1;                       // the wave leaves its line column
				}
			}
			if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = ph; best_seen = seen; best_bad = bad; }
		}
		groups_seen[horizontal ? 0 : 1] = best_seen; groups_straddling[horizontal ? 0 : 1] = best_bad;
		return best;
	};
	// rows: local row ly maps to frame row gy; with bands of a multiple of 8 rows (or one band) gy = ly + const (mod 8)
	const uint32_t gy0 = a.p.band_first * a.p.band_rows;
	a.phase_x = best_phase(true, a.p.x0, a.p.out_width, gy0 + std::min(a.p.out_rows, a.p.band_rows) / 2u);
	a.phase_y = best_phase(false, gy0, a.p.out_rows < a.p.band_rows ? a.p.out_rows : a.p.band_rows, a.p.x0 + a.p.out_width / 2u);
	if (!axis_aligned || groups_seen[0] + groups_seen[1] == 0) return 1000u;
	// One screen direction clean, the other not (pose (90,0,0): the rows of pixels sit on cell boundaries of the axis that carries the
	// 4e-8 of rounding noise, 9 % of the 2x2 blocks straddle; the columns are clean): TRILINEAR puts the four lanes of a quad along the
	// CLEAN direction — measured on that pose 2.49 -> 2.24 ms (scripts/phase_grid_probe.py); with both directions clean the 2x2 blocks
	// stay (2.11 against 2.16 ms on pose (0,0,0)).  What is returned is the share of straddling groups of the lane order chosen.
	if (!nearest && groups_seen[0] > 0 && groups_seen[1] > 0) {
		const bool dirty_x = groups_straddling[0] * 50 > groups_seen[0], dirty_y = groups_straddling[1] * 50 > groups_seen[1];     // > 2 %
		if (dirty_y && !dirty_x) { a.lane_map = kLaneRows; return (uint32_t) (groups_straddling[0] * 1000 / groups_seen[0]); }
		if (dirty_x && !dirty_y) { a.lane_map = kLaneColumns; return (uint32_t) (groups_straddling[1] * 1000 / groups_seen[1]); }
	}
	return (uint32_t) ((groups_straddling[0] + groups_straddling[1]) * 1000 / (groups_seen[0] + groups_seen[1]));
}

// Moves c->completed_seq forward over every frame whose stop event has been reached (frames complete out of order across streams:
// the mark only passes a frame once all earlier ones are done too — conservative, which is what recycling a buffer needs).
void advance_completed(vr_ctx *c) {
	while (c->completed_seq + 1 < c->seq_next) {
		const uint64_t next = c->completed_seq + 1;
		const int slot = (int) ((c->ring_head + kEventRing - (int) ((c->seq_next - next) % kEventRing)) % kEventRing);
		if (c->seq_next - next < (uint64_t) kEventRing && c->ring_seq[slot] == next && c->ring[slot].pending) {
			const hipError_t q = hipEventQuery(c->ring[slot].stop);
			if (q != hipSuccess) { (void) hipGetLastError(); break; }
		}                                            // (an entry that was overwritten or harvested since belongs to a finished frame)
		c->completed_seq = next;
	}
}

// kLayoutRunDual, the product's rule (no history needed): which run copy the tiles of every block of workgroup tiles read, from the
// cube face the block's centre ray enters through.  All lanes of a wave start ON that face and march in lockstep, so a wave's samples
// lie in a plane parallel to it: the runs should lie IN that plane (lanes that are neighbours along the run axis then read the same
// 36-byte run, and the wave touches fewer lines per step) — entry through a z face -> runs along y, through a y face -> runs along z,
// through an x face -> runs along y.  Measured (scripts/gpu_r04_c.sh, full march, four oblique orthogonal poses, ms): this rule 2.76 /
// 2.88 / 2.82 / 2.99; the round-3 MEASURED per-block choice (four set-up frames per parameter set) 2.80 / 2.94 / 2.88 / 2.96; one copy
// for the whole frame 3.18-3.54; the other seven face -> copy tables 2.85-4.0 (x face -> runs along z: 2.85 / 2.86 / 3.05 / 2.95).
// vr_hip_set_brick_plane(6) keeps the measured choice as the validator.  Where a block's centre ray misses the cube other tiles of
// the block are tried; a block that misses everywhere keeps the frame's default.  Blocks are groups of 64 consecutive tile numbers =
// the 8x8-tile blocks of the tile numbering (larger groups for huge frames: at most 1024 bits travel in the kernel argument).
void dual_choice_bits(RayKernelArgs &a, const RaymarchPlan &plan, bool default_alt) {
	const vr_view &v = a.p.view;
	const uint32_t ntiles = plan.tiles_x * plan.tiles_y;
	uint32_t shift = 6;                                            // 64 consecutive tile numbers = one 8x8-tile block (tile_number_to_xy)
	while (((ntiles + (1u << shift) - 1u) >> shift) > 32u * kDualWords) shift++;
	const uint32_t groups = (ntiles + (1u << shift) - 1u) >> shift;
	const float tile_w = 32.0f, tile_h = 16.0f;                     // the 512-thread workgroup tile of the table-addressed variants
	memset(a.dual_bits, 0, sizeof a.dual_bits);
	// tuning aid: VR_DUAL_RULE = 3-bit mask, bit f set = tiles entered through a face of axis f (0 x, 1 y, 2 z) read the copy along y
	static const int rule = [] { const char *e = getenv("VR_DUAL_RULE"); return e ? atoi(e) : -1; }();
	auto entry_choice = [&](float px, float py, bool &alt) -> bool {          // pixel of the tile grid -> does its ray hit, and which copy
		const float lxf = std::fmin(std::fmax(px - (float) a.phase_x, 0.0f), (float) (a.p.out_width - 1u));
		const float lyf = std::fmin(std::fmax(py - (float) a.phase_y, 0.0f), (float) (a.p.out_rows - 1u));
		const uint32_t ly = (uint32_t) lyf, band = ly / a.p.band_rows;
		const uint32_t gy = (band * a.p.band_stride + a.p.band_first) * a.p.band_rows + (ly - band * a.p.band_rows);
		const float fx = (float) ((int) (a.p.x0 + (uint32_t) lxf) - (int) (v.width / 2u)), fy = (float) ((int) gy - (int) (v.height / 2u));
		float o[3], d[3], k_in[3], k_out[3];
		for (int i = 0; i < 3; i++) {
			o[i] = v.perspective ? v.origin[i] : v.origin[i] + v.right_plane[i] * fx + v.up_plane[i] * fy;
			d[i] = v.perspective ? v.direction[i] + v.right_plane[i] * fx + v.up_plane[i] * fy : v.direction[i];
			if (d[i] != 0.0f) { const float k1 = (-1.0f - o[i]) / d[i], k2 = (1.0f - o[i]) / d[i]; k_in[i] = std::fmin(k1, k2); k_out[i] = std::fmax(k1, k2); }
			else { k_in[i] = -3.0e38f; k_out[i] = std::fabs(o[i]) <= 1.0f ? 3.0e38f : -3.0e38f; }
		}
		const float kin = std::fmax(std::fmax(k_in[0], k_in[1]), k_in[2]), kout = std::fmin(std::fmin(k_out[0], k_out[1]), k_out[2]);
		if (!(kin < kout && kout > 0.0f)) return false;
		const int face = (k_in[2] >= k_in[0] && k_in[2] >= k_in[1]) ? 2 : (k_in[1] >= k_in[0] ? 1 : 0);
		alt = rule >= 0 ? ((rule >> face) & 1) != 0 : face != 1;
		return true;
	};
	for (uint32_t g = 0; g < groups; g++) {
		// the centre of the group's tiles first (tile 27 of 64 = column 3, row 3 of an 8x8 block: next to the block's centre), then a spread of the others
		const uint32_t first = g << shift, count = std::min(1u << shift, ntiles - first);
		static const uint32_t probe[9] = { 27, 36, 9, 14, 49, 54, 0, 63, 31 };
		bool alt = default_alt;
		for (int i = 0; i < 9; i++) {
			const uint32_t t = first + (uint32_t) (((uint64_t) probe[i] * count) >> 6);
			uint32_t tx = 0, ty = 0;
			tile_number_to_xy(t, plan.tiles_x, plan.tiles_y, &tx, &ty);
			const float cx = ((float) tx + (probe[i] == 27 ? 1.0f : 0.5f)) * tile_w, cy = ((float) ty + (probe[i] == 27 ? 1.0f : 0.5f)) * tile_h;
			bool a_i;
			if (entry_choice(cx, cy, a_i)) { alt = a_i; break; }
		}
		if (alt) a.dual_bits[g >> 5] |= 1u << (g & 31u);
	}
	a.dual_analytic = 1u; a.dual_shift = shift;
}

// the part of the kernel argument that only restates the frame parameters and the geometry of the resident volume
void volume_args(const vr_ctx *c, const vr_params *p, RayKernelArgs &a) {
	memset(&a, 0, sizeof a);
	a.p = *p;
	a.dim_x = c->dim[0]; a.dim_y = c->dim[1]; a.dim_z = c->dim[2];
	a.stride_y = c->dim[0]; a.stride_z = (uint64_t) c->dim[0] * c->dim[1];
	a.half_x = 0.5f * (float) c->dim[0]; a.half_y = 0.5f * (float) c->dim[1]; a.half_z = 0.5f * (float) c->dim[2];
	a.off_x = a.half_x - 0.5f; a.off_y = a.half_y - 0.5f; a.off_z = a.half_z - 0.5f;
	a.max_x = (float) (c->dim[0] - 1); a.max_y = (float) (c->dim[1] - 1); a.max_z = (float) (c->dim[2] - 1);
	a.lh_x = 0.01f * a.half_x; a.lh_y = 0.01f * a.half_y; a.lh_z = 0.01f * a.half_z;
	a.tf_scale = c->bpv == 1 ? (float) VR_TF_SIZE / 255.0f : (float) VR_TF_SIZE / 65535.0f;
	a.kd_scaled = p->light_kd * (c->bpv == 1 ? (1.0f / 255.0f) : (1.0f / 65535.0f));
	a.tf_zero_below = c->tf_zero_below;
	a.nbx = (c->dim[0] + kBrickEdge - 1) / kBrickEdge; a.nby = (c->dim[1] + kBrickEdge - 1) / kBrickEdge;
	a.nbz = (c->dim[2] + kBrickEdge - 1) / kBrickEdge;
	if (c->clip_on) {
		a.clip_on = 1u;
		for (int i = 0; i < 3; i++) { a.clip_min[i] = c->clip.box_min[i]; a.clip_max[i] = c->clip.box_max[i]; }
		for (int i = 0; i < 4; i++) a.clip_plane[i] = c->clip.plane[i];
	} else {
		// the identity clip, which changes no bit of a segment by contract: what the kernels that always run clip_segment read when no clip
		// is set (raymarch_shadowed, composite_lit); clip_on stays 0 and every other kernel ignores these words
		for (int i = 0; i < 3; i++) { a.clip_min[i] = -1.0f; a.clip_max[i] = 1.0f; }
	}
}

// the corner test of the transparent-sample shortcut (RayKernelArgs::skip_mask / skip_cmp) for the resident transfer function: the largest
// power of two P with fma(P, tf_scale, -0.5) <= tf_zero_below — raw < P implies a transparent sample
// (zero_below: the leading all-zero entries of the function the frame classifies with — the resident one's, or a tf2d table's envelope's)
void transparent_corner_test(const vr_ctx *c, RayKernelArgs &a, float zero_below) {
	uint32_t below = 0;
	const uint32_t top = c->bpv == 1 ? 256u : 65536u;
	for (uint32_t P = 1; P <= top; P <<= 1)
		if (zero_below >= 0.0f && std::fmaf((float) P, a.tf_scale, -0.5f) <= zero_below) below = P;
	a.skip_cmp = below == 0 ? 1u : 0u;
	if (below == 0) a.skip_mask = 0u;
	else if (c->bpv == 1) a.skip_mask = ((0xffu & ~(below - 1u)) * 0x01010101u);
	else a.skip_mask = ((0xffffu & ~(below - 1u)) * 0x00010001u);
}
void transparent_corner_test(const vr_ctx *c, RayKernelArgs &a) { transparent_corner_test(c, a, c->tf_zero_below); }

// index / block edge of the ESL grid, prepared as shift or multiply-high (RaycasterBase.h:59-63)
void esl_divisor(RayKernelArgs &a, uint32_t block_dims) {
	const uint32_t bd = block_dims ? block_dims : 1u;
	if ((bd & (bd - 1)) == 0) { a.esl_div_magic = 0; a.esl_div_shift = (uint32_t) __builtin_ctz(bd); }
	else { a.esl_div_magic = (uint32_t) ((1ull << 32) / bd + 1); a.esl_div_shift = 0; }
}

// What vr_hip_set_run_flavour(0), the automatic choice, gives a full-march frame that reads run bricks: the aligned flavour (true) or the
// nine-element runs (false).  Measured (profiles/run7_ab.txt): the eight-view cycle 1.821 -> 1.747 ms per frame, the five run-brick views -2 .. -10 %.
constexpr bool kRunAutoAligned = true;

// ---- what launch_frame and launch_full_march_frame (further down; its copy choice, full_march_copy, also serves build_shadow) decide the same way ----

// the copy a frame of this layout reads (not asked for kLayoutLinear)
uint32_t copy_kind_of(const RayKernelArgs &a, uint32_t sampling) {
	if (is_run_layout((int) a.layout) && a.run_aligned) return a.layout == kLayoutRunY ? kCopyRun7Y : kCopyRun7Z;
	return a.layout == kLayoutRun || a.layout == kLayoutRunDual ? kCopyRunZ : a.layout == kLayoutRunY ? kCopyRunY : a.layout == kLayoutVoxel ? kCopyVoxel :
	       a.layout == kLayoutOct ? kCopyOct : a.layout == kLayoutColumn ? (sampling == VR_SAMPLE_NEAREST ? kCopyColVoxX : kCopyColX) + a.col_axis :
	       a.layout == kLayoutVoxCol ? kCopyColVoxX + a.col_axis : kCopyQuadXY + a.brick_plane;
}

// d = |direction * half| (cells per unit of k along every volume axis), its major axis — ties go to the higher axis — and whether the
// view, or in perspective its central direction, runs along that axis
struct ViewAxis { float d[3]; int major; bool along; };
ViewAxis view_axis(const vr_params *p, const float *half) {
	ViewAxis v;
	for (int i = 0; i < 3; i++) v.d[i] = std::fabs(p->view.direction[i] * half[i]);
	const float dx = v.d[0], dy = v.d[1], dz = v.d[2];
	v.major = dz >= dx && dz >= dy ? 2 : (dy >= dx ? 1 : 0);
	v.along = std::fmax(dx, std::fmax(dy, dz)) > 0.98f * std::sqrt(dx * dx + dy * dy + dz * dz);
	return v;
}
// the chunk plane across a volume axis
uint32_t plane_across(int axis) { return axis == 2 ? kPlaneXY : (axis == 1 ? kPlaneXZ : kPlaneYZ); }

// neighbouring pixels are at most one cell apart along every volume axis
bool one_cell_per_pixel(const vr_params *p, const float *half) {
	for (int ax = 0; ax < 3; ax++)
		if ((std::fabs(p->view.right_plane[ax]) + std::fabs(p->view.up_plane[ax])) * half[ax] > 1.0f) return false;
	return true;
}

// TRILINEAR with 2-byte voxels: the oct bricks (one 16-byte gather per sample instead of two 8-byte ones) for ORTHOGONAL views
// with at most one cell per pixel — there the pixels of a lane quad share their elements and the halved gather count wins
// (1024^3: 4.0 / 5.8 / 4.0 / 4.2 ms against 5.1 / 6.0 / 5.9 / 5.6 with the quad bricks; 2048^3: 28-44 against 40-48 ms); the
// rays of a perspective view diverge to more than a cell per pixel, every lane then pulls 16 bytes it uses once, and the doubled
// traffic loses (4.2-5.5 against 3.5-4.4 ms): those keep the quad bricks.  Not when a quad copy is forced (testing) or the
// index-arithmetic path is.
bool takes_oct_bricks(const vr_ctx *c, const vr_params *p, const float *half) {
	if (p->sampling == VR_SAMPLE_NEAREST || c->bpv != 2 || c->layout != VR_LAYOUT_BRICKED || !copy_possible(c, kCopyOct) || c->brick_plane_force >= 0 || c->force_wide == 1 ||
	    (p->view.perspective && !c->oct_always))
		return false;
	return c->oct_always || one_cell_per_pixel(p, half);
}

// No copy could be built: any resident copy this sampling mode can read (the run copies only for a caller whose kernel reads them), else
// the linear array.  Sets the layout and returns the copy.
const void *resident_fallback(const vr_ctx *c, uint32_t sampling, bool run_copies, uint32_t &layout) {
	const bool nearest = sampling == VR_SAMPLE_NEAREST;
	if (nearest && c->copy[kCopyVoxel] && c->force_wide != 1) { layout = kLayoutVoxel; return c->copy[kCopyVoxel]; }
	if (run_copies && !nearest && !c->force_wide && c->copy[kCopyRunZ]) { layout = kLayoutRun; return c->copy[kCopyRunZ]; }
	if (run_copies && !nearest && !c->force_wide && c->copy[kCopyRunY]) { layout = kLayoutRunY; return c->copy[kCopyRunY]; }
	if (!nearest && c->bpv == 2 && c->force_wide != 1 && c->copy[kCopyOct]) { layout = kLayoutOct; return c->copy[kCopyOct]; }
	layout = kLayoutLinear;
	return nullptr;
}

// In-cube sample coordinates are exact to ~2^-23 * (1 + 2 max|origin|) * N/2 texels; the unclamped fetch (vr_march.h)
// needs them inside (-1, N), i.e. an error below 1/2.  True with a factor-4 margin.
float max_abs_origin(const vr_params *p) { return std::fmax(std::fabs(p->view.origin[0]), std::fmax(std::fabs(p->view.origin[1]), std::fabs(p->view.origin[2]))); }
bool fetch_coordinates_exact(const vr_ctx *c, const vr_params *p) { return (1.0f + 2.0f * max_abs_origin(p)) * (float) max_dim_of(c) < 1048576.0f; }

// cost[ntiles] and order[ntiles * order_words_per_tile] for at least `ntiles` tiles.  Buffers that are too small are freed (nothing of them
// may be in flight) and allocated anew; false, with none left, if that fails.
bool ensure_tile_buffers(uint32_t *&cost, uint32_t *&order, uint32_t &capacity, uint32_t ntiles, uint32_t order_words_per_tile) {
	if (capacity >= ntiles) return true;
	if (cost) { (void) hipFree(cost); (void) hipFree(order); cost = order = nullptr; capacity = 0; }
	if (hipMalloc((void **) &cost, (size_t) ntiles * 4) == hipSuccess && hipMalloc((void **) &order, (size_t) ntiles * 4 * order_words_per_tile) == hipSuccess) { capacity = ntiles; return true; }
	(void) hipGetLastError();
	if (cost) (void) hipFree(cost);
	cost = order = nullptr;
	return false;
}

// cached lane orders / tile phases were chosen for another volume, copy or plane
void forget_tile_mappings(vr_ctx *c) { c->map_cached = 0; c->map_next = 0; }
// recorded tile orders describe other ray lengths or another scheduling mode (buffers and last-use marks stay: recycled only when free)
void forget_recorded_orders(vr_ctx *c) {
	for (auto &e : c->map_cache) { e.dual_state = 0; e.order_tiles = 0; }
	for (auto &e : c->order_cache) { e.has_last = false; e.repeats = 0; for (auto &sl : e.slot) sl.valid = false; }
}

// refuses a call that needs the linear array once that was released; `remedy` ends the message
int need_linear(vr_ctx *c, const char *remedy) {
	if (c->vol != nullptr || c->dim[0] == 0) return VR_OK;
	return fail(c, VR_ERR_NOT_READY, (std::string("the linear copy was released (vr_hip_release_linear_copy): ") + remedy).c_str());
}

// the event pair and the sequence number of the frame about to be launched (only blocks if kEventRing launches are still in flight)
EventPair &next_frame_events(vr_ctx *c, uint64_t &frame_seq) {
	EventPair &ev = c->ring[c->ring_head];
	frame_seq = c->seq_next++;
	c->ring_seq[c->ring_head] = frame_seq;
	c->ring_head = (c->ring_head + 1) % kEventRing;
	harvest(c, ev);
	return ev;
}

#ifdef VR_BOUNDS_CHECK
// debug build: what the frame's gathers must stay inside, and where the first violation is recorded
hipError_t bounds_check_arm(vr_ctx *c, RayKernelArgs &a, const vr_params *p, const RaymarchPlan &plan, const void *brick_copy, uint32_t ntiles) {
	if (c->bc_fault == nullptr) {
		hipError_t e = hipMalloc((void **) &c->bc_fault, 8 * sizeof(uint32_t));
		if (e == hipSuccess) e = hipMemset(c->bc_fault, 0, 8 * sizeof(uint32_t));
		if (e != hipSuccess) return e;
	}
	const void *array = plan.reads_linear ? c->vol : brick_copy;
	const bool column = a.layout == kLayoutColumn || a.layout == kLayoutVoxCol;
	a.bc_base = (uint64_t) (uintptr_t) array - (column ? kColPadBytes : 0u);
	a.bc_bytes = plan.reads_linear ? (c->vol_elems + volume_tail_slack(c->dim[0], c->dim[1])) * c->bpv :
	             copy_bytes(c, copy_kind_of(a, p->sampling));
	if (column) a.bc_bytes += 2ull * kColPadBytes;
	a.bc_alt_bytes = a.alt_copy ? copy_bytes(c, a.layout == kLayoutVoxCol ? kCopyColX + a.col_axis : (uint32_t) (a.run_aligned ? kCopyRun7Y : kCopyRunY)) : 0;      // (the pair fetch never reads the padding)
	a.bc_fault = c->bc_fault; a.bc_ntiles = ntiles;
	// self-test of the net itself: VR_BC_SELFTEST=1 halves the size the checks hold the gathers against — a full-march frame must then fail
	if (const char *e = getenv("VR_BC_SELFTEST")) if (atoi(e) == 1) a.bc_bytes /= 2;
	return hipSuccess;
}

// ... and what the frame recorded: waits for it
int bounds_check_verdict(vr_ctx *c, hipStream_t stream, uint32_t layout) {
	uint32_t fault[6] = { 0, 0, 0, 0, 0, 0 };
	VR_TRY(c, hipStreamSynchronize(stream));
	VR_TRY(c, hipMemcpy(fault, c->bc_fault, sizeof fault, hipMemcpyDeviceToHost));
	if (fault[0] != 0u) {
		char msg[256];
		snprintf(msg, sizeof msg, "bounds check: code %u (1 table index [axis << 8], 2 offset, 3 address, 4 cost slot) workgroup %u thread %u value 0x%08x%08x limit %u, layout %u",
		         fault[0], fault[1], fault[2], fault[4], fault[3], fault[5], layout);
		(void) hipMemset(c->bc_fault, 0, 8 * sizeof(uint32_t));
		return fail(c, VR_ERR_HIP, msg);
	}
	return VR_OK;
}
#endif

// One frame: `launch` between the start and stop events of the frame's pair, armed before and judged after in the bounds-checked build.
// frame_seq = the frame's sequence number.
template <class Launch>
int launch_timed(vr_ctx *c, RayKernelArgs &a, const vr_params *p, const RaymarchPlan &plan, const void *brick_copy, hipStream_t stream, uint64_t &frame_seq, Launch &&launch) {
#ifdef VR_BOUNDS_CHECK
	VR_TRY(c, bounds_check_arm(c, a, p, plan, brick_copy, plan.tiles_x * plan.tiles_y));
#endif
	EventPair &ev = next_frame_events(c, frame_seq);
	VR_TRY(c, hipEventRecord(ev.start, stream));
	VR_TRY(c, launch());
	VR_TRY(c, hipEventRecord(ev.stop, stream));
	ev.pending = true;
#ifdef VR_BOUNDS_CHECK
	{ const int bc = bounds_check_verdict(c, stream, a.layout); if (bc) return bc; }
#endif
	return VR_OK;
}

int build_shadow(vr_ctx *c);

// the refusal of NEAREST by the five kinds of frame that are defined on the interpolated field, `what` in the message (launch_frame words its own)
int need_interpolated(vr_ctx *c, const vr_params *p, const char *what) {
	if (p->sampling == VR_SAMPLE_TRILINEAR || p->sampling == VR_SAMPLE_TRILINEAR_Q8) return VR_OK;
	return fail(c, VR_ERR_INVALID, (std::string(what) + " is defined on the interpolated field: sampling must be VR_SAMPLE_TRILINEAR or VR_SAMPLE_TRILINEAR_Q8").c_str());
}

// the lighting and shadow words of the kernel argument, from what vr_hip_set_lighting and vr_hip_set_shadow left in the context (the light
// grid is built by then: build_shadow)
void lighting_shadow_args(const vr_ctx *c, RayKernelArgs &a) {
	if (c->lighting_on) {
		a.light_on = 1u; a.light_ka = c->lighting.ambient; a.light_kd = c->lighting.diffuse; a.light_ks = c->lighting.specular;
		a.light_n = c->lighting.shininess_log2;
	}
	if (c->shadow_on) {
		const uint32_t S = c->shadow.dims;
		a.shadow_on = 1u; a.shadow_last = S - 2u; a.shadow_hs = 0.5f * (float) (S - 1u); a.shadow_max = (float) (S - 1u);
		a.shadow_scale = c->shadow.strength * (1.0f / 255.0f); a.shadow_base = 1.0f - c->shadow.strength;
		a.shadow_row = S; a.shadow_slab = S * S; a.shadow_q = (uint64_t) (uintptr_t) c->shadow_q;
	}
}

// What the copy steps of launch_frame hand on.  run_layout: which run copy a run-brick frame reads — runs along z unless the view marches along z;
// hit, straddle: the cached tile mapping (none under a forced mapping and for a backdrop frame) and the straddle figure; dual_stage, measured /
// alternating choice only: -1 no; 0..3: the four frames before; 4: per-tile choice in use
struct CopyChoice { uint32_t run_layout = kLayoutRun, straddle = 1000u; vr_ctx::MapEntry *hit = nullptr; bool dual_analytic = false, shade_pairs = false; int dual_stage = -1; };
// (a shadowed, lit, pre-integrated or backdrop frame reads what a clipped frame reads: its kernels are the clipped ones with more per dense sample)
bool clipped_frame(const vr_ctx *c, const RayKernelArgs &a) { return c->clip_on || c->shadow_on || c->lighting_on || c->preint_on || a.backdrop_on; }

// a.layout and a.brick_plane by view, sampling mode and the forced planes, then the tile mapping, which may still move the frame to another copy
int choose_composite_copy(vr_ctx *c, const vr_params *p, const ViewAxis &va, RayKernelArgs &a, CopyChoice &choice) {
	const bool bricked = c->layout == VR_LAYOUT_BRICKED, clip = clipped_frame(c, a);
	a.layout = bricked ? kLayoutBricked : kLayoutLinear;
	bool run_candidate = false, run_if_unaligned = false, dual_candidate = false;
	vr_ctx::MapEntry *&hit = choice.hit;
	// Which brick copy: the one whose 16-byte chunks lie in the plane perpendicular to the view's dominant axis, so that the
	// pixels of a lane quad — neighbours on the screen — are neighbours inside a chunk (TRILINEAR; NEAREST keeps (x,y)).
	// Copies are built on first use (copy_for, further down); copy_possible asks without building.
	a.brick_plane = kPlaneXY;
	if (p->sampling != VR_SAMPLE_NEAREST && bricked && !c->force_wide) {
		uint32_t plane = kPlaneXY;
		if (c->brick_plane_force >= 0) plane = (uint32_t) c->brick_plane_force;
		else {
			// only for views (or, in perspective, central directions) along a volume axis: measured on the oblique benchmark pose the
			// (x,y) copy is as good as any (4.1 ms against 4.1 - 5.1 ms), along an axis the perpendicular plane wins by 8 - 16 %
			if (va.major == 2 && copy_possible(c, kCopyRunY)) choice.run_layout = kLayoutRunY;     // runs across the march, never along it
			if (va.along) {
				plane = plane_across(va.major);
				// Perspective along x or y: the pixel pitch grows from 0.4 to 1.1 cells along the march, most lane quads straddle
				// chunks, and the run bricks — whose runs (along z) then lie across the march — are faster (measured 2.08 / 2.18 ms
				// against 2.49 / 2.51 ms on the benchmark poses).  Along z the runs lie along the march and the quad copy wins
				// (2.48 against 2.99 ms).  Orthogonal views along an axis are decided below, from how well their quads can be aligned.
				if (p->view.perspective && (plane != kPlaneXY || choice.run_layout == kLayoutRunY)) run_candidate = true;
				else if (!p->view.perspective) run_if_unaligned = true;
			} else {
				run_candidate = true;       // not along an axis: lane quads straddle chunks whatever the plane -> one 8-byte gather
				// ... and which run copy is better depends on the cube face a tile's rays enter through (kLayoutRunDual).  Orthogonal
				// views only: on the oblique perspective pose the two copies are level almost everywhere (per-tile best of both -3 %)
				// and mixing them costs that much again (2.60 -> 2.62-2.64 ms); on the orthogonal one 3.20 -> 2.81 ms.
				dual_candidate = !p->view.perspective;
			}
		}
		if (plane == kPlanes + 3 || plane == kPlanes + 4) { run_candidate = true; dual_candidate = true; }     // forced: 6 = measured per-tile choice, 7 = alternating tiles
		// a clipped frame reads no run copy (there is no clipped kernel for them): the quad copy of the view's plane, (x,y) where a run copy is forced
		if (clip) { run_candidate = run_if_unaligned = dual_candidate = false; if (plane >= kPlanes) plane = kPlaneXY; }
		if (plane < kPlanes && copy_possible(c, kCopyQuadXY + plane)) a.brick_plane = plane;
		else if (plane == kPlanes && copy_possible(c, kCopyRunZ)) a.layout = kLayoutRun;               // forced: 3 = runs along z, 4 = runs along y
		else if (plane == kPlanes + 1 && copy_possible(c, kCopyRunY)) a.layout = kLayoutRunY;
		if (run_candidate && copy_possible(c, choice.run_layout == kLayoutRunY ? kCopyRunY : kCopyRunZ)) a.layout = choice.run_layout;
	}
	// NEAREST: the voxel bricks (one voxel per element) unless a quad copy is forced (testing) or a 64-bit path is
	if (p->sampling == VR_SAMPLE_NEAREST && bricked && copy_possible(c, kCopyVoxel) && c->brick_plane_force < 0 && c->force_wide != 1)
		a.layout = kLayoutVoxel;
	const float half[3] = { a.half_x, a.half_y, a.half_z };
	if (takes_oct_bricks(c, p, half)) a.layout = kLayoutOct;
	esl_divisor(a, p->esl_block_dims);

	if (c->tile_lane_map >= 0) { a.lane_map = (uint32_t) c->tile_lane_map; a.phase_x = c->tile_phase_x; a.phase_y = c->tile_phase_y; }
	else if (a.backdrop_on) choice.straddle = choose_tile_mapping(a);      // a backdrop frame leaves the cached mappings alone: they are keyed by vr_params, and it reads other copies
	else {
		for (uint32_t i = 0; i < c->map_cached && hit == nullptr; i++)
			if (memcmp(&c->map_cache[i].p, p, sizeof *p) == 0 && memcmp(c->map_cache[i].dim, c->dim, sizeof c->dim) == 0) hit = &c->map_cache[i];
		if (hit == nullptr) {
			const uint32_t straddle = choose_tile_mapping(a);
			hit = &c->map_cache[c->map_next];
			hit->straddle_permille = straddle;
			// the recycled entry's measured copy choice belonged to other parameters; frames that read or record its buffers may still be
			// in flight on other streams — the validator is a testing aid, so it simply waits for them
			if (hit->dual_state != 0 || hit->order_tiles != 0) VR_TRY(c, drain(c));
			hit->dual_state = 0; hit->order_tiles = 0;
			constexpr uint32_t kMaps = sizeof c->map_cache / sizeof c->map_cache[0];
			c->map_next = (c->map_next + 1) % kMaps;
			if (c->map_cached < kMaps) c->map_cached++;
			hit->p = *p; memcpy(hit->dim, c->dim, sizeof c->dim);
			hit->lane_map = a.lane_map; hit->phase_x = a.phase_x; hit->phase_y = a.phase_y;
		}
		a.lane_map = hit->lane_map; a.phase_x = hit->phase_x; a.phase_y = hit->phase_y;
		choice.straddle = hit->straddle_permille;
		// An orthogonal view along an axis whose pixels sit exactly on cell boundaries can carry rounding noise in its direction
		// (pose (180,90,0): components of 4e-8) that moves boundary pixels to the other neighbour part-way along the ray and
		// differently across the frame: no phase aligns it.  Measured on that pose: 3.18 ms with the run bricks against 3.71 ms.
		if (run_if_unaligned && hit->straddle_permille > 150u && copy_possible(c, choice.run_layout == kLayoutRunY ? kCopyRunY : kCopyRunZ)) a.layout = choice.run_layout;
	}
	// Per-tile choice between the two run copies (kLayoutRunDual, vr_device.h): full-march frames only (with leaping or early
	// termination the rays are short and the tile order is what matters), never for the clamping instantiation (its clamp bounds are
	// per axis, and the tile's y / z exchange would have to reach them).  The product's rule is ANALYTIC and needs no earlier frame:
	// every tile picks its copy in the kernel from the cube face the centre ray of its block of tiles enters through (raymarch_kernel)
	// — the first frame of a new view already reads the right copies.  vr_hip_set_brick_plane(6) keeps the round-3 MEASURED choice
	// (frames 0-3 of a parameter set on one copy each, the last two recording tile costs, choice kernel, per-block choice from frame 4 on)
	// as the validator of that rule; 7 = alternating tiles (testing: the copies meet at tile boundaries all over the frame).
	const bool dual_test = c->brick_plane_force == (int) kPlanes + 4, dual_measured = c->brick_plane_force == (int) kPlanes + 3;
	if (dual_candidate && is_run_layout(a.layout) && !p->esl && p->ray_threshold >= 1.0f && !a.clamp_fetch && c->bpv == 1 &&
	    copy_possible(c, kCopyRunZ) && copy_possible(c, kCopyRunY)) {
		if (dual_test || dual_measured) {
			if (hit != nullptr && c->tile_scheduling == 1 && !VR_ORDER_ALWAYS) {
				choice.dual_stage = dual_test ? 4 : (int) hit->dual_state;
				a.layout = choice.dual_stage == 4 ? kLayoutRunDual : ((choice.dual_stage & 1) ? kLayoutRunY : kLayoutRun);
			}
		} else {
			choice.dual_analytic = true;
			a.layout = kLayoutRunDual;
		}
	}
	return VR_OK;
}

// Column windows (kLayoutColumn, vr_device.h): full-march TRILINEAR frames of ORTHOGONAL views along a volume axis — every ray stays in
// one cell column (at most one cell flip per lateral axis: the direction's other components are rounding noise), all rays share the k
// sequence, and colmarch_kernel marches on wave-uniform state: one 16-byte gather and one transparency test per ~3 samples.  What the
// host checks: the lateral drift over the longest possible segment stays below half a cell, a sample advances between 1/64 and 1 cell
// along the axis (the kernel re-checks both per wave and otherwise marches per lane), at most one cell per pixel (the 32-bit offsets
// of a wave's columns), no clamping instantiation.  Measured on the benchmark poses (full march, lit): 2.12 / 2.13 / 2.86 ms before.
// NEAREST takes the same march over windows of 16 plain voxels (colmarch_nearest_kernel, kCopyColVox*): one gather per sixteen samples.
// Early ray termination alone is fine (the kernels clear a terminated lane's live bit like the general one; the k sequence stays shared);
// such frames give up the measured-cost tile order, which the column kernels do not take.
void column_march(const vr_ctx *c, const vr_params *p, const ViewAxis &va, RayKernelArgs &a, CopyChoice &choice) {
	static const bool col_ert = [] { const char *e = getenv("VR_COL_ERT"); return e == nullptr || atoi(e) != 0; }();      // VR_COL_ERT=0: A/B
	// Not a clipped frame: the column kernels march the whole cube on state the rays of a wave share, and a clipped segment is per ray.
	if (!(c->layout == VR_LAYOUT_BRICKED && !clipped_frame(c, a) && c->bpv == 1 && !c->force_wide && !p->view.perspective && !p->esl && (p->ray_threshold >= 1.0f || col_ert) &&
	      !a.clamp_fetch && c->column_force >= 0 && (c->brick_plane_force < 0 || c->column_force > 0)))
		return;
	const float half[3] = { a.half_x, a.half_y, a.half_z };
	const float *d = va.d;
	const int m = va.major;
	const float advance = d[m] * p->ray_step;
	bool take = advance >= 1.0f / 64.0f && advance <= 1.0f && one_cell_per_pixel(p, half);
	if (c->column_force == 0)                                          // per view: along the axis — 4 > 2 sqrt(3), the longest segment in k
		for (int i = 0; i < 3; i++) if (i != m && d[i] * 4.0f >= 0.45f) take = false;
	// TRILINEAR reads the voxel windows (kLayoutVoxCol, voxcol_tri_kernel) where every wave's rectangle of cell columns fits in its 64
	// lanes: along a lateral axis i the 8x8 pixels of a wave span 7 pixel steps, i.e. at most floor(7 * cells per step) + 2 cells, + 1
	// for the +1 neighbours of a trilinear sample and + 1 for a column flip.  The quad-element windows (colmarch_kernel) otherwise.
	const bool nearest = p->sampling == VR_SAMPLE_NEAREST;
	bool voxcol = false;
	if (!nearest && c->column_copy != 1u && col_copy_bytes(c->dim, (uint32_t) m, true) < (1ull << 32)) {      // (the kernel's explicit fetches use 32-bit offsets)
		auto span = [&](int i) { return (int) std::floor(7.0f * (std::fabs(p->view.right_plane[i]) + std::fabs(p->view.up_plane[i])) * half[i]) + 4; };
		voxcol = span(m == 0 ? 1 : 0) * span(m == 2 ? 1 : 2) <= 64;
	}
	if (!take || !copy_possible(c, (nearest || voxcol ? kCopyColVoxX : kCopyColX) + (uint32_t) m)) return;
	a.layout = voxcol ? kLayoutVoxCol : kLayoutColumn; a.col_axis = (uint32_t) m; a.brick_plane = (uint32_t) m;
	// the dense path's constants, grouped for one scalar load each (vr_device.h); the products are the device's own fp32 products
	a.col_sample.ax = p->view.direction[0] * a.half_x; a.col_sample.ay = p->view.direction[1] * a.half_y; a.col_sample.az = p->view.direction[2] * a.half_z;
	a.col_sample.tf_scale = a.tf_scale; a.col_sample.tf_zero_below = a.tf_zero_below;
	a.col_sample.max_x = a.max_x; a.col_sample.max_y = a.max_y; a.col_sample.max_z = a.max_z;
	a.col_sample.light_kd = p->light_kd; a.col_sample.ray_threshold = p->ray_threshold;
	for (int i = 0; i < 3; i++) { a.col_shade.dir[i] = p->view.direction[i]; a.col_shade.light[i] = p->view.light_pos[i]; }
	a.col_shade.lh[0] = a.lh_x; a.col_shade.lh[1] = a.lh_y; a.col_shade.lh[2] = a.lh_z;
	a.col_shade.kd_scaled = a.kd_scaled;
	for (int i = 0; i < 3; i++) a.col_shade.dim[i] = c->dim[i];
	a.col_shade.nbu = col_blocks(c->dim[m == 0 ? 1 : 0]);
	a.col_shade.nw = col_windows(c->dim[m], nearest || voxcol ? kColVoxCells : kColCells);
	a.col_shade.nwq = col_windows(c->dim[m]);
	// a lit voxel-window frame shades from the quad-element windows of the same axis (voxcol_pairs_kernel: one 8-byte load per shaded
	// sample instead of eight byte loads) — a second copy of 16/3 bytes per voxel, which vr_hip_set_column_copy(2) declines
	choice.shade_pairs = voxcol && p->light_kd > 0.01f && c->column_copy == 0;
	choice.dual_analytic = false; choice.dual_stage = -1;
}

// The copy this frame reads, built now if this is its first use.  A build that is refused (HBM guard, allocation, linear array
// released) degrades to the next best resident copy; the image is the same.
const void *acquire_copies(vr_ctx *c, const vr_params *p, CopyChoice &choice, RayKernelArgs &a) {
	const void *brick_copy = nullptr;
	// Run bricks, full march (the condition of kLayoutRunDual: with leaping or early termination the rays are short, and those frames keep
	// the copies they have): the ALIGNED flavour (vr_device.h kRun7*: no run straddles a cache line) where the copies the frame would read
	// are resident or can be built — same tiles, same copy per tile, same lane maps and wave shapes, same image; vr_hip_set_run_flavour.
	// A build that is refused leaves the frame on the nine-element runs.
	if (is_run_layout((int) a.layout) && !p->esl && p->ray_threshold >= 1.0f && c->bpv == 1 && (c->run_flavour == 2u || (c->run_flavour == 0u && kRunAutoAligned))) {
		const bool want_z = a.layout != kLayoutRunY, want_y = a.layout != kLayoutRun;
		if ((!want_z || copy_possible(c, kCopyRun7Z)) && (!want_y || copy_possible(c, kCopyRun7Y))) {
			const void *cz = want_z ? copy_for(c, kCopyRun7Z) : nullptr, *cy = want_y ? copy_for(c, kCopyRun7Y) : nullptr;
			if ((!want_z || cz != nullptr) && (!want_y || cy != nullptr)) {
				a.run_aligned = 1u;
				brick_copy = want_z ? cz : cy;
				if (a.layout == kLayoutRunDual) a.alt_copy = (uint64_t) (uintptr_t) cy;
			}
		}
	}
	if (a.layout == kLayoutRunDual && brick_copy == nullptr) {
		brick_copy = copy_for(c, kCopyRunZ);
		a.alt_copy = (uint64_t) (uintptr_t) copy_for(c, kCopyRunY);
		if (brick_copy == nullptr || a.alt_copy == 0) { a.layout = choice.run_layout; choice.dual_stage = -1; choice.dual_analytic = false; brick_copy = nullptr; }
	}
	if (a.layout != kLayoutLinear && brick_copy == nullptr) {
		const uint32_t want = copy_kind_of(a, p->sampling);
		brick_copy = copy_for(c, want);
		if (brick_copy == nullptr && want != kCopyQuadXY) {
			a.layout = kLayoutBricked; a.brick_plane = kPlaneXY;
			forget_tile_mappings(c);                         // lane orders were chosen for the copy that could not be had
			brick_copy = copy_for(c, kCopyQuadXY);
		}
		if (brick_copy == nullptr) brick_copy = resident_fallback(c, p->sampling, !clipped_frame(c, a), a.layout);      // no quad copy either
	}
	// ... and the copy its shading samples read.  Refused or impossible (as above): the frame shades by byte loads from the voxel windows
	if (choice.shade_pairs && a.layout == kLayoutVoxCol && brick_copy != nullptr) a.alt_copy = (uint64_t) (uintptr_t) copy_for(c, kCopyColX + a.col_axis);
	return brick_copy;
}

// no frame that may still run reads or records the slot, and its order kernel, if one was issued, has run: its buffers may be rewritten
bool slot_idle(const vr_ctx *c, const vr_ctx::SchedSlot &sl) {
	if (sl.last_seq > c->completed_seq) return false;
	if (sl.ready != nullptr && sl.issue_seq != 0 && hipEventQuery(sl.ready) != hipSuccess) { (void) hipGetLastError(); return false; }
	return true;
}

// bd: the opaque layer of a backdrop frame (vr_hip_render_backdrop_device; device addresses), or NULL
int launch_frame(vr_ctx *c, const vr_params *p, void *dev_rgba, hipStream_t stream, const vr_backdrop *bd = nullptr) {
	// A shadowed frame (vr_hip_set_shadow): the light grid first, on the context's stream and synchronous like a brick copy's first use
	const bool nearest = p->sampling == VR_SAMPLE_NEAREST;
	if (c->shadow_on && nearest)
		return fail(c, VR_ERR_INVALID, "a shadow is set: the light grid and its factor are defined on the interpolated field — sampling must be VR_SAMPLE_TRILINEAR or "
		                               "VR_SAMPLE_TRILINEAR_Q8 (vr_hip_set_shadow(ctx, NULL) switches the shadow off)");
	if (c->shadow_on) if (const int rc = build_shadow(c)) return rc;
	// A gradient-lit, a pre-integrated and a backdrop frame read what a clipped frame reads too; clip, shadow, lighting and pre-integration compose
	if (c->lighting_on && nearest)
		return fail(c, VR_ERR_INVALID, "a lighting is set: the gradient is defined on the interpolated field — sampling must be VR_SAMPLE_TRILINEAR or "
		                               "VR_SAMPLE_TRILINEAR_Q8 (vr_hip_set_lighting(ctx, NULL) switches the lighting off)");
	if (c->preint_on && nearest)
		return fail(c, VR_ERR_INVALID, "pre-integration is set: a slab lies between two samples of the interpolated field — sampling must be VR_SAMPLE_TRILINEAR or "
		                               "VR_SAMPLE_TRILINEAR_Q8 (vr_hip_set_preintegration(ctx, 0) switches it off)");
	if (bd != nullptr && nearest)
		return fail(c, VR_ERR_INVALID, "a backdrop frame is defined on the interpolated field — sampling must be VR_SAMPLE_TRILINEAR or VR_SAMPLE_TRILINEAR_Q8");
	RayKernelArgs a;
	volume_args(c, p, a);
	if (c->preint_on) a.slab_on = 1u;
	if (bd != nullptr) { a.backdrop_on = 1u; a.backdrop_rgba = (uint64_t) (uintptr_t) bd->rgba; a.backdrop_depth = (uint64_t) (uintptr_t) bd->depth; }
	lighting_shadow_args(c, a);
	const float half[3] = { a.half_x, a.half_y, a.half_z };
	const ViewAxis va = view_axis(p, half);
	transparent_corner_test(c, a);
	// fp32 sample coordinates that are not exact to a fraction of a cell: clamp every sample
	const float omax = max_abs_origin(p), nmax = (float) max_dim_of(c);
	a.clamp_fetch = fetch_coordinates_exact(c, p) ? 0u : 1u;
	// intersect() replaces a direction component that is exactly 0 by 1e-5 (RaycasterBase.h:33-35): a ray whose origin lies
	// up to ky * 1e-5 outside a face of the cube is then still reported as a hit and marches at that constant out-of-cube
	// coordinate, ky * 1e-5 * N/2 texels beyond the face.  ky <= sqrt(3) * (omax + 1) for |direction| >= 1 (orthogonal: unit
	// direction; perspective: a unit vector plus in-plane offsets).  Keep that below 1/8 texel, else clamp every sample.
	if (1.7321f * (omax + 1.0f) * 1e-5f * nmax * 0.5f >= 0.125f) a.clamp_fetch = 1u;
	// The unclamped march fetches up to kDepth steps past a ray's exit point (software pipeline): that must stay inside the
	// kLutPad repeated edge entries of the address tables.  The reference's longest step is 1.666 cells (RaycasterBase.cpp:90).
	// A step moves a ray by ray_step * |direction component| * N/2 cells along an axis; perspective directions are not
	// normalised (direction + right * fx + up * fy, ViewBase.h:29-31), so the bound is taken over the whole frame.
	float advance = 0.0f;
	for (int i = 0; i < 3; i++) {
		float d = std::fabs(p->view.direction[i]);
		if (p->view.perspective)
			d += std::fabs(p->view.right_plane[i]) * (0.5f * (float) p->view.width + 1.0f) + std::fabs(p->view.up_plane[i]) * (0.5f * (float) p->view.height + 1.0f);
		advance = std::fmax(advance, d * half[i]);
	}
	if (!((float) kOverrunSteps * p->ray_step * advance + 1.5f <= (float) kLutPad)) a.clamp_fetch = 1u;
	if (c->force_clamp_fetch & 1u) a.clamp_fetch = 1u;
	auto pow2 = [](uint32_t n) { return n != 0 && (n & (n - 1)) == 0; };
	a.near_scaled = (pow2(c->dim[0]) && pow2(c->dim[1]) && pow2(c->dim[2]) && !(c->force_clamp_fetch & 2u)) ? 1u : 0u;
	a.force_wide = c->force_wide;
	CopyChoice choice;
	if (const int rc = choose_composite_copy(c, p, va, a, choice)) return rc;
	column_march(c, p, va, a, choice);
	const void *brick_copy = acquire_copies(c, p, choice, a);
	// Shape of a wave's pixel tile (8x8, 16x4 or 4x16 inside the 32x16-pixel workgroup tile): a perspective view along a volume axis
	// that reads run bricks gets its waves elongated along the screen direction the RUNS map to — the lanes of a wave then share the
	// 36-byte runs (and their cache lines) instead of spreading over twice as many cell columns.  Measured on the benchmark's
	// perspective poses: 2.07 -> 1.96 (along z, runs along y: tall), 2.04 -> 1.95 (along y, runs along z: tall), 2.05 -> 1.96 ms
	// (along x, runs along z: wide); oblique views and orthogonal views lose 3-9 % with either elongated shape and keep 8x8.
	if (c->tile_lane_map < 0 && is_run_layout(a.layout) && p->view.perspective && !p->esl && va.along) {       // (with leaping the rays are short: no difference measured)
		const int run_axis = a.layout == kLayoutRunY ? 1 : 2;
		const float across = std::fabs(p->view.right_plane[run_axis]), down = std::fabs(p->view.up_plane[run_axis]);
		a.lane_map = (a.lane_map & 3u) | ((down > across ? 2u : 1u) << 2);
	}
	// NEAREST on voxel bricks, perspective view along x or y: the four lanes of a quad are four pixels along the screen direction that
	// maps to z — four different slices, i.e. four different lines — not a 2x2-pixel block: byte gathers whose lanes fall into the same
	// dwords serialise (measured on the benchmark poses: 1.44 -> 1.38 ms along y, 1.46 -> 1.38 ms along x; along z the blocks stay: 1.23).
	if (c->tile_lane_map < 0 && a.layout == kLayoutVoxel && p->view.perspective && (a.lane_map & 3u) == kLaneBlocks && va.major != 2)
		a.lane_map = std::fabs(p->view.up_plane[2]) > std::fabs(p->view.right_plane[2]) ? kLaneColumns : kLaneRows;
	const RaymarchPlan plan = plan_raymarch(a, brick_copy != nullptr, c->bpv);
	if (plan.reads_linear && c->vol == nullptr)
		return fail(c, VR_ERR_NOT_READY, "this frame needs the linear array, which was released (vr_hip_release_linear_copy): no resident brick copy "
		                                 "serves this sampling mode / addressing path — prepare it before releasing, or set the volume again");
	const uint32_t ntiles = plan.tiles_x * plan.tiles_y;
	if (choice.dual_analytic && a.layout == kLayoutRunDual) dual_choice_bits(a, plan, choice.run_layout == kLayoutRunY);
	// Measured-cost launch order: only where rays differ in length (empty-space leaping or early termination on) — the full
	// march has no tail to remove and keeps its cache-friendly tile numbering.
	TileSchedule sched;
	vr_ctx::SchedSlot *read_slot = nullptr, *record_slot = nullptr;
	vr_ctx::OrderEntry *oe = nullptr;
	// (not a backdrop frame: the layer changes per frame and the recorded orders are keyed by vr_params — its tiles start in grid order)
	if (c->tile_scheduling == 1 && c->tile_lane_map < 0 && !a.backdrop_on && (VR_ORDER_ALWAYS || p->esl || p->ray_threshold < 1.0f) && ntiles >= 64 && ntiles <= (1u << 20)) {
		advance_completed(c);
		vr_ctx::OrderKey key;
		memset(&key, 0, sizeof key);
		key.sampling = p->sampling; key.esl = p->esl ? 1u : 0u; key.ert = p->ray_threshold < 1.0f ? 1u : 0u; key.perspective = p->view.perspective ? 1u : 0u;
		const int m = va.major;
		key.major_axis = (uint32_t) m * 2u + (p->view.direction[m] < 0.0f ? 1u : 0u);
		// ... and the direction itself in steps of 1/8 per component (views within a few degrees share their costs, different poses do not)
		const float len = std::sqrt(p->view.direction[0] * p->view.direction[0] + p->view.direction[1] * p->view.direction[1] + p->view.direction[2] * p->view.direction[2]);
		for (int i = 0; i < 3; i++) key.direction_q[i] = len > 0.0f ? (int32_t) std::lrint(p->view.direction[i] / len * 8.0f) : 0;
		key.layout = a.layout; key.view_w = p->view.width; key.view_h = p->view.height; key.x0 = p->x0; key.out_width = p->out_width; key.out_rows = p->out_rows;
		key.band_rows = p->band_rows; key.band_stride = p->band_stride; key.band_first = p->band_first;
		memcpy(key.dim, c->dim, sizeof key.dim); key.tiles_x = plan.tiles_x; key.tiles_y = plan.tiles_y;
		vr_ctx::OrderEntry *lru = &c->order_cache[0];        // an unused entry if there is one, else the least recently used
		for (auto &e : c->order_cache) {
			if (e.used && memcmp(&e.key, &key, sizeof key) == 0) { oe = &e; break; }
			if (lru->used && (!e.used || e.lru < lru->lru)) lru = &e;
		}
		if (oe == nullptr) {                         // new policy key: take the least recently used entry; its slots keep their buffers and their last-use marks
			oe = lru;
			oe->used = true; oe->key = key; oe->has_last = false; oe->repeats = 0;
			for (auto &sl : oe->slot) sl.valid = false;
		}
		oe->lru = c->seq_next;
		// the order this frame launches in: the most recently issued one that has FINISHED (or was issued on this very stream, which orders it
		// before this frame); only when there is none, one still being built on another stream, behind a device-side wait
		vr_ctx::SchedSlot *pending_elsewhere = nullptr;
		for (auto &sl : oe->slot) {
			if (!sl.valid || sl.ntiles != ntiles) continue;
			bool usable = sl.stream == stream;
			if (!usable) { const hipError_t q = hipEventQuery(sl.ready); if (q == hipSuccess) usable = true; else (void) hipGetLastError(); }
			if (usable) { if (read_slot == nullptr || sl.issue_seq > read_slot->issue_seq) read_slot = &sl; }
			else if (pending_elsewhere == nullptr || sl.issue_seq > pending_elsewhere->issue_seq) pending_elsewhere = &sl;
		}
		if (read_slot == nullptr && pending_elsewhere != nullptr) {
			VR_TRY(c, hipStreamWaitEvent(stream, pending_elsewhere->ready, 0));
			read_slot = pending_elsewhere;
		}
		// No order at all — the first frame under this policy key (a new view: the reference's benchmark renders every view once): predict
		// the tile costs from the ESL bit volume (tile_estimate_kernel) and order by them, on this stream, in front of the frame
		static const bool estimate = [] { const char *e = getenv("VR_TILE_ESTIMATE"); return e == nullptr || atoi(e) != 0; }();      // VR_TILE_ESTIMATE=0: A/B
		if (read_slot == nullptr && estimate && p->esl && a.layout != kLayoutColumn && a.layout != kLayoutVoxCol) {
			vr_ctx::SchedSlot *est = nullptr;
			for (auto &sl : oe->slot)
				if (slot_idle(c, sl)) { est = &sl; break; }
			if (est != nullptr && !ensure_tile_buffers(est->cost, est->order, est->capacity, ntiles, 1u)) est = nullptr;
			if (est != nullptr) {
				if (est->ready == nullptr) VR_TRY(c, hipEventCreateWithFlags(&est->ready, hipEventDisableTiming));
				RayKernelArgs ea = a;
				ea.tiles_x = plan.tiles_x; ea.tiles_y = plan.tiles_y;
				VR_TRY(c, launch_tile_estimate(ea, plan.tile_h, c->esl, est->cost, ntiles, stream));
				VR_TRY(c, launch_tile_order(est->cost, est->order, ntiles, stream));
				VR_TRY(c, hipEventRecord(est->ready, stream));
				est->valid = true; est->ntiles = ntiles; est->stream = stream; est->issue_seq = c->seq_next;
				read_slot = est;
			}
		}
		if (read_slot != nullptr) sched.order = read_slot->order;
		// record this frame's tile costs?  Always while the parameters keep changing (a moving camera: the next frame's order comes from
		// this one), twice for a frame that is repeated unchanged (the first recording of a view may have run on cold caches)
		const bool same = oe->has_last && memcmp(&oe->last, p, sizeof *p) == 0;
		if (!same) { oe->last = *p; oe->has_last = true; oe->repeats = 0; }
		if (oe->repeats < 2u) {
			for (auto &sl : oe->slot) {
				if (&sl == read_slot || !slot_idle(c, sl)) continue;                     // in use by this frame / by a frame that may still run / its order kernel has not run yet
				if (record_slot == nullptr || (!sl.valid && record_slot->valid) || (sl.valid == record_slot->valid && sl.issue_seq < record_slot->issue_seq)) record_slot = &sl;
			}
			if (record_slot != nullptr && !ensure_tile_buffers(record_slot->cost, record_slot->order, record_slot->capacity, ntiles, 1u)) record_slot = nullptr;      // (free: nothing of it is in flight)
			if (record_slot != nullptr) {
				if (record_slot->ready == nullptr) VR_TRY(c, hipEventCreateWithFlags(&record_slot->ready, hipEventDisableTiming));
				record_slot->valid = false;
				VR_TRY(c, hipMemsetAsync(record_slot->cost, 0, (size_t) ntiles * 4, stream));
				sched.cost = record_slot->cost;
			}
		}
	}
	// kLayoutRunDual by the measured / alternating choice: frames 2 and 3 record, frame 3 is followed by the choice kernel, frame 4 onwards reads
	// the choice.  Every step is ordered behind the one before through the entry's event when it runs on another stream.
	vr_ctx::MapEntry *hit = choice.hit;
	const bool dual_test = c->brick_plane_force == (int) kPlanes + 4;
	if (choice.dual_stage >= 0) {
		if (ntiles < 2u || ntiles > (1u << 20)) choice.dual_stage = -1;      // (a frame that keeps kLayoutRunDual without a choice reads the copy along z)
		else if (hit->capacity < ntiles) {
			if (hit->cost) VR_TRY(c, drain(c));
			if (!ensure_tile_buffers(hit->cost, hit->order, hit->capacity, ntiles, 2u)) choice.dual_stage = -1;      // (order: the choice, and behind it the second recording)
			if (!dual_test) { hit->dual_state = 0; if (choice.dual_stage > 0) choice.dual_stage = -1; }      // (cannot happen: the grid of a parameter set does not change)
		}
	}
	if (choice.dual_stage >= 0) {
		if (hit->order_ready == nullptr) VR_TRY(c, hipEventCreateWithFlags(&hit->order_ready, hipEventDisableTiming));
		if (choice.dual_stage > 0 && !(dual_test && hit->order_tiles != ntiles) && hit->order_stream != nullptr && stream != hit->order_stream)
			VR_TRY(c, hipStreamWaitEvent(stream, hit->order_ready, 0));
		if (dual_test) {                                   // alternating tiles, built once per grid size
			if (hit->order_tiles != ntiles) {
				VR_TRY(c, launch_tile_choice(nullptr, nullptr, hit->order, ntiles, stream));
				VR_TRY(c, hipEventRecord(hit->order_ready, stream));
				hit->order_tiles = ntiles; hit->order_stream = stream;
			}
			sched.order = hit->order;
		} else if (choice.dual_stage == 2 || choice.dual_stage == 3) {
			uint32_t *into = choice.dual_stage == 2 ? hit->cost : hit->order + hit->capacity;
			VR_TRY(c, hipMemsetAsync(into, 0, (size_t) ntiles * 4, stream));
			sched.cost = into;
		} else if (choice.dual_stage == 4) sched.order = hit->order;
	}
	if (c->tile_scheduling == 2 && ntiles <= (1u << 20)) {     // profiling: the cost of every tile of this frame, tile = workgroup id
		if (const int rc = grow_buffer(c, (void **) &c->cost_map, c->cost_map_bytes, (size_t) ntiles * 4)) return rc;
		VR_TRY(c, hipMemsetAsync(c->cost_map, 0, (size_t) ntiles * 4, stream));
		sched.cost = c->cost_map;
		c->cost_map_tiles_x = plan.tiles_x; c->cost_map_tiles_y = plan.tiles_y;
	}

	// (the TRILINEAR column march over the voxel windows reports layout 7, the column march, and column_voxels = 1; column_shade_pairs = 1
	// when it shades from the quad-element windows)
	c->last_launch = vr_launch_info{ a.layout == kLayoutVoxCol ? (uint32_t) kLayoutColumn : a.layout, a.brick_plane, a.lane_map, a.phase_x, a.phase_y, a.clamp_fetch,
	                                 plan.tiles_x, plan.tiles_y, sched.order != nullptr ? 1u : 0u, choice.straddle,
	                                 a.layout == kLayoutVoxCol ? 1u : 0u, a.layout == kLayoutVoxCol && a.alt_copy != 0 ? 1u : 0u, c->shadow_on ? 1u : 0u };
	c->last_run_flavour = is_run_layout((int) a.layout) && brick_copy != nullptr ? (a.run_aligned ? 2u : 1u) : 0u;

	uint64_t frame_seq = 0;
	const int rc = launch_timed(c, a, p, plan, brick_copy, stream, frame_seq, [&] { return launch_raymarch(a, c->vol, brick_copy, c->bpv, c->tf, c->esl, dev_rgba, sched, stream); });
	if (rc) return rc;
	if (c->lighting_on) c->lit_frames++;
	if (c->preint_on) c->preint_frames++;
	if (bd != nullptr) c->backdrop_frames++;
	if (choice.dual_stage >= 0 && choice.dual_stage < 4) {      // behind the frame, on its stream: the entry moves to its next stage
		if (choice.dual_stage == 3) VR_TRY(c, launch_tile_choice(hit->cost, hit->order + hit->capacity, hit->order, ntiles, stream));
		VR_TRY(c, hipEventRecord(hit->order_ready, stream));
		hit->order_stream = stream; hit->order_tiles = ntiles;
		hit->dual_state = (uint32_t) choice.dual_stage + 1u;
	}
	if (read_slot != nullptr) read_slot->last_seq = frame_seq;
	if (record_slot != nullptr) {                // behind the frame, on its stream: the order for the next frame under this policy key
		VR_TRY(c, launch_tile_order(record_slot->cost, record_slot->order, ntiles, stream));
		VR_TRY(c, hipEventRecord(record_slot->ready, stream));
		record_slot->valid = true; record_slot->ntiles = ntiles; record_slot->stream = stream; record_slot->issue_seq = record_slot->last_seq = frame_seq;
		oe->repeats++;
	}
	return VR_OK;
}

int ready(vr_ctx *c) {
	bool any = c->vol != nullptr;
	for (uint32_t k = 0; k < kCopySlots; k++) any = any || c->copy[k] != nullptr;
	if (!any) return fail(c, VR_ERR_NOT_READY, "render before set_volume");
	if (!c->tf_set) return fail(c, VR_ERR_NOT_READY, "render before set_transfer_fn");
	return VR_OK;
}

// Waits for every frame this context has queued (on its own or on callers' streams) and for its own stream: what the reference's
// synchronous set_* calls imply, without stalling other contexts or streams of the device (no hipDeviceSynchronize).
hipError_t drain(vr_ctx *c) {
	for (int i = 0; i < kEventRing; i++)
		if (c->ring[i].pending) { hipError_t e = hipEventSynchronize(c->ring[i].stop); if (e != hipSuccess) return e; }
	return hipStreamSynchronize(c->stream);
}

void free_bricks(vr_ctx *c) {
	for (uint32_t k = 0; k < kCopySlots; k++) {
		if (c->copy[k]) { (void) hipFree(k >= kCopyColX && k <= kCopyColVoxZ ? (uint8_t *) c->copy[k] - kColPadBytes : (uint8_t *) c->copy[k]); c->copy[k] = nullptr; }
		c->copy_build_ms[k] = 0; c->copy_failed[k] = false;
	}
}

uint64_t copy_bytes(const vr_ctx *c, uint32_t kind) {
	if (kind <= kCopyQuadYZ) return bricked_elems(c->dim[0], c->dim[1], c->dim[2]) * 4 * c->bpv;
	if (kind == kCopyVoxel) return bricked_elems(c->dim[0], c->dim[1], c->dim[2]) * c->bpv;
	if (kind == kCopyOct) return bricked_elems(c->dim[0], c->dim[1], c->dim[2]) * 8 * c->bpv;
	if (kind >= kCopyColX && kind <= kCopyColZ) return col_copy_bytes(c->dim, kind - kCopyColX);
	if (kind >= kCopyColVoxX && kind <= kCopyColVoxZ) return col_copy_bytes(c->dim, kind - kCopyColVoxX, true);
	if (kind == kCopyRun7Z) return run7_copy_bytes(c->dim[0], c->dim[1], c->dim[2]);
	if (kind == kCopyRun7Y) return run7_copy_bytes(c->dim[0], c->dim[2], c->dim[1]);
	return run_copy_bytes(c->dim[0], c->dim[1], c->dim[2]);
}

// does the layout policy have this copy at this volume size at all?  (quad (x,y): always; the other planes and the run bricks:
// 1-byte voxels, edges the 32-bit tables cover; voxel bricks: wherever the address tables reach)
bool copy_in_policy(const vr_ctx *c, uint32_t kind) {
	if (c->layout != VR_LAYOUT_BRICKED || c->dim[0] == 0) return false;
	if (kind == kCopyQuadXY) return true;
	if (kind == kCopyVoxel) return max_dim_of(c) <= 2048u;
	if (kind == kCopyOct) return c->bpv == 2 && max_dim_of(c) <= 2048u;
	if (kind >= kCopyColX && kind <= kCopyColVoxZ) return c->bpv == 1 && max_dim_of(c) <= 2048u;
	if (kind == kCopyQuadXZ || kind == kCopyQuadYZ) return c->bpv == 1 && max_dim_of(c) <= 1024u && copy_bytes(c, kind) <= (1ull << 32);
	return c->bpv == 1 && max_dim_of(c) <= 1024u;
}

// resident, or buildable on first use (the policy has it, the linear array is still there, no earlier build was refused)
bool copy_possible(const vr_ctx *c, uint32_t kind) {
	if (c->copy[kind]) return true;
	return copy_in_policy(c, kind) && c->vol != nullptr && !c->copy_failed[kind];
}

// Builds copy `kind` from the linear array on the context's stream and waits for it (a one-time stall of the first frame that
// wants it: 6-8 ms per copy at 1024^3).  Every copy but the first quad copy is only built while half of the HBM stays free.
int build_copy(vr_ctx *c, uint32_t kind) {
	if (c->copy[kind]) return VR_OK;
	if (!copy_possible(c, kind)) return VR_ERR_NOT_READY;
	const uint64_t bytes = copy_bytes(c, kind);
	// the half-of-the-HBM rule exempts the ONE copy a sampling mode cannot do without: the first quad copy — for 2-byte voxels the oct
	// copy, which TRILINEAR reads instead (building both is left to a caller who forces the quad copy: testing)
	if (kind != kCopyQuadXY && !(kind == kCopyOct && c->copy[kCopyQuadXY] == nullptr)) {
		size_t free_b = 0, total_b = 0;
		if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes >= free_b || free_b - bytes < total_b / 2) { (void) hipGetLastError(); c->copy_failed[kind] = true; return VR_ERR_ALLOC; }
	}
	void *dst = nullptr;
	const bool column = kind >= kCopyColX && kind <= kCopyColVoxZ;       // column windows: zeroed padding in front and behind (vr_device.h kColPadBytes)
	if (hipMalloc(&dst, bytes + (column ? 2ull * kColPadBytes : 0ull)) != hipSuccess) { (void) hipGetLastError(); c->copy_failed[kind] = true; return fail(c, VR_ERR_ALLOC, "brick copy allocation failed"); }
	hipError_t e = hipSuccess;
	if (column) {
		e = hipMemsetAsync(dst, 0, kColPadBytes, c->stream);
		if (e == hipSuccess) e = hipMemsetAsync((uint8_t *) dst + kColPadBytes + bytes, 0, kColPadBytes, c->stream);
		dst = (uint8_t *) dst + kColPadBytes;                            // what kernels and downloads see; free_bricks undoes the offset
	}
	if (e == hipSuccess) e = hipEventRecord(c->aux_start, c->stream);
	if (e == hipSuccess) {
		if (kind <= kCopyQuadYZ) e = launch_brickify(c->vol, dst, c->bpv, kind - kCopyQuadXY, c->dim[0], c->dim[1], c->dim[2], c->stream);
		else if (kind == kCopyVoxel) e = launch_brickify_voxel(c->vol, dst, c->bpv, c->dim[0], c->dim[1], c->dim[2], c->stream);
		else if (kind == kCopyOct) e = launch_brickify_oct(c->vol, dst, c->dim[0], c->dim[1], c->dim[2], c->stream);
		else if (kind >= kCopyColX && kind <= kCopyColZ) e = launch_build_column(c->vol, dst, kind - kCopyColX, false, c->dim[0], c->dim[1], c->dim[2], c->stream);
		else if (kind >= kCopyColVoxX && kind <= kCopyColVoxZ) e = launch_build_column(c->vol, dst, kind - kCopyColVoxX, true, c->dim[0], c->dim[1], c->dim[2], c->stream);
		else e = launch_brickify_run(c->vol, dst, kind == kCopyRunY || kind == kCopyRun7Y ? kLayoutRunY : kLayoutRun, kind >= kCopyRun7Z, c->dim[0], c->dim[1], c->dim[2], c->stream);
	}
	if (e == hipSuccess) e = hipEventRecord(c->aux_stop, c->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
	if (e != hipSuccess) { (void) hipGetLastError(); (void) hipFree(column ? (uint8_t *) dst - kColPadBytes : (uint8_t *) dst); c->copy_failed[kind] = true; return fail(c, VR_ERR_HIP, "brick copy build failed", e); }
	(void) hipEventElapsedTime(&c->copy_build_ms[kind], c->aux_start, c->aux_stop);
	c->copy[kind] = dst;
	return VR_OK;
}

const void *copy_for(vr_ctx *c, uint32_t kind) {
	if (c->copy[kind] == nullptr) (void) build_copy(c, kind);
	return c->copy[kind];
}

// the labels belong to one volume (and one set of dims): nothing of them may be in flight here
void drop_labels(vr_ctx *c) {
	if (c->labels) { (void) hipFree(c->labels); c->labels = nullptr; }
	if (c->label_bricks) { (void) hipFree(c->label_bricks); c->label_bricks = nullptr; }
	c->label_bricks_failed = false;
}

// field B belongs to one volume (its dims and voxel size): nothing of it may be in flight here.  Its function and the fused bits stay.
void drop_second(vr_ctx *c) {
	if (c->second) { (void) hipFree(c->second); c->second = nullptr; }
	for (int k = 0; k < 4; k++) {
		if (c->second_copy[k]) { (void) hipFree(c->second_copy[k]); c->second_copy[k] = nullptr; }
		c->second_copy_failed[k] = false;
	}
}

int alloc_volume(vr_ctx *c, uint32_t x, uint32_t y, uint32_t z, uint32_t bpv) {
	if (x == 0 || y == 0 || z == 0 || x > 65535u || y > 65535u || z > 65535u)       // Model::dims is ushort3
		return fail(c, VR_ERR_INVALID, "volume dims out of range (1..65535)");
	if (bpv != 1 && bpv != 2) return fail(c, VR_ERR_INVALID, "bytes_per_voxel must be 1 or 2");
	VR_TRY(c, drain(c));                         // frames still reading the volume we are about to free
	if (c->vol) { (void) hipFree(c->vol); c->vol = nullptr; }
	free_bricks(c);
	drop_labels(c);                              // vr_hip_set_labels: the labels go with the volume they were set for
	drop_second(c);                              // vr_hip_set_second_volume: ... and so does field B
	forget_tile_mappings(c);                     // cached tile mappings belong to the previous volume
	c->mip_mapped = 0; c->mip_map_next = 0; c->mip_bounds_ready = false;       // ... and so do the block maxima of the MIP frames
	c->shadow_ready = false;                     // ... and the light grid of a shadow
	c->dim[0] = c->dim[1] = c->dim[2] = 0;
	const uint64_t elems = (uint64_t) x * y * z;
	const uint64_t slack = volume_tail_slack(x, y);
	VR_TRY(c, hipMalloc(&c->vol, (elems + slack) * bpv));
	VR_TRY(c, hipMemsetAsync((uint8_t *) c->vol + elems * bpv, 0, slack * bpv, c->stream));
	c->vol_elems = elems; c->dim[0] = x; c->dim[1] = y; c->dim[2] = z; c->bpv = bpv;
	return VR_OK;
}

// voxels per edge of an ESL block of the resident volume (RaycasterBase.cpp:97-99)
uint32_t volume_block_dims(const vr_ctx *c) {
	const uint32_t bd = (max_dim_of(c) + VR_ESL_VOLUME_DIMS - 1) / VR_ESL_VOLUME_DIMS;
	return bd < VR_ESL_MIN_BLOCK ? VR_ESL_MIN_BLOCK : bd;
}

// The bounds a MIP frame skips by (vr_device.h): the min/max scan of the linear array and the small kernel behind it, on the
// context's stream, synchronous like a brick copy's first use.  Kept until the volume changes.
int build_mip_bounds(vr_ctx *c) {
	if (c->mip_bounds_ready) return VR_OK;
	if (c->vol == nullptr)
		return fail(c, VR_ERR_NOT_READY, "the block maxima of a MIP frame with esl on are built from the linear array, which was released before the first such frame");
	if (c->mip_bounds == nullptr) VR_TRY(c, hipMalloc((void **) &c->mip_bounds, kMipBoundBytes));
	VR_TRY(c, launch_minmax(c->vol, c->bpv, c->dim[0], c->dim[1], c->dim[2], volume_block_dims(c), c->minmax, c->stream));
	VR_TRY(c, launch_mip_bounds(c->minmax, c->mip_bounds, c->stream));
	VR_TRY(c, hipStreamSynchronize(c->stream));
	c->mip_bounds_ready = true;
	return VR_OK;
}

// The copy a full-march frame of params p reads, and with it a.layout and a.brick_plane: voxel bricks for NEAREST, quad bricks for TRILINEAR
// (oct bricks for 2-byte voxels where a DVR frame takes them), the linear array (NULL) under VR_LAYOUT_LINEAR; a copy that is refused falls
// back to the first quad copy, then to whatever is resident.  plane_force is read as vr_ctx::brick_plane_force is: below 0 = the chunk plane
// across a view along a volume axis, 0..2 = that plane (and no voxel bricks).  Also what build_shadow reads, for its own params and plane.
// force_linear: the answer under VR_LAYOUT_LINEAR whatever the context's layout is (a fused frame whose second field has no such copy).
const void *full_march_copy(vr_ctx *c, const vr_params *p, int32_t plane_force, RayKernelArgs &a, bool force_linear = false) {
	const float half[3] = { a.half_x, a.half_y, a.half_z };
	const bool bricked = c->layout == VR_LAYOUT_BRICKED && !force_linear, nearest = p->sampling == VR_SAMPLE_NEAREST, forced = plane_force >= 0 && plane_force < (int32_t) kPlanes;
	a.force_wide = c->force_wide;
	a.layout = bricked ? kLayoutBricked : kLayoutLinear;
	a.brick_plane = kPlaneXY;
	if (bricked && nearest && copy_possible(c, kCopyVoxel) && c->force_wide != 1 && !forced)
		a.layout = kLayoutVoxel;
	if (bricked && !nearest && !c->force_wide) {
		uint32_t plane = kPlaneXY;
		if (forced) plane = (uint32_t) plane_force;
		else if (plane_force < 0) {                      // along a volume axis: the chunk plane across it
			const ViewAxis va = view_axis(p, half);
			if (va.along) plane = plane_across(va.major);
		}
		if (copy_possible(c, kCopyQuadXY + plane)) a.brick_plane = plane;
	}
	if (!force_linear && takes_oct_bricks(c, p, half)) a.layout = kLayoutOct;
	if (a.layout == kLayoutLinear) return nullptr;
	const void *brick_copy = copy_for(c, copy_kind_of(a, p->sampling));
	if (brick_copy == nullptr) {                         // refused or not buildable any more: the first quad copy, then whatever is resident
		a.layout = kLayoutBricked; a.brick_plane = kPlaneXY;
		brick_copy = copy_for(c, kCopyQuadXY);
	}
	if (brick_copy == nullptr) brick_copy = resident_fallback(c, p->sampling, false, a.layout);      // (these frames never read the run copies)
	return brick_copy;
}

// What a caller of launch_full_march_frame asks for: `what` names the frame in messages; block_maxima: params.esl skips fetches by the
// volume's block maxima (MIP, isosurface) — without it the frame is planned and cached as the same frame with esl off; leaping: the kernel
// argument carries the composite's leaping instead (params.esl, the divisor of params.esl_block_dims, the transparent-sample test: depth,
// labelled); plane: a chunk plane that stands in for the context's forced plane, -1 = as the context says; second_field: the frame reads the
// context's second field in the order of the copy it reads of the volume (fused) — where that copy of the field cannot be had
// (second_copy_for), the frame is planned as a VR_LAYOUT_LINEAR frame: both from their linear arrays.
struct FullMarch { const char *what; bool block_maxima, leaping; int32_t plane; bool second_field = false; };
const void *second_copy_for(vr_ctx *c, uint32_t layout, uint32_t plane);

// One frame that marches every ray in full — MIP, isosurface, section, depth, labelled: the copy it reads (full_march_copy), the block maxima
// where it skips by them, the tile mapping of a DVR frame of the same view, one launch, one event pair.  launch(a, brick_copy, bounds or
// NULL) starts the kernel; it may add words of its own to a.
template <class Launch>
int launch_full_march_frame(vr_ctx *c, const vr_params *params, hipStream_t stream, const FullMarch &f, Launch &&launch) {
	vr_params planned = *params;
	if (!f.block_maxima) planned.esl = 0u;
	const vr_params *p = &planned;
	RayKernelArgs a;
	volume_args(c, p, a);
	const void *brick_copy = full_march_copy(c, p, f.plane >= 0 ? f.plane : c->brick_plane_force, a);
	if (f.second_field && brick_copy != nullptr && second_copy_for(c, a.layout, a.brick_plane) == nullptr)
		brick_copy = full_march_copy(c, p, f.plane >= 0 ? f.plane : c->brick_plane_force, a, true);
	// Skipping and stopping by block maxima.  The grid is the volume's own (vr_hip_volume_minmax), whatever params.esl_block_* say.  Not
	// for views so far away that fp32 sample coordinates are not exact to a small fraction of a cell (the condition under which DVR
	// frames clamp every fetch, launch_frame): the TRILINEAR bound covers one voxel around the block of the sample's position.
	esl_divisor(a, volume_block_dims(c));
	if (p->esl && !fetch_coordinates_exact(c, p)) a.p.esl = 0u;
	if (a.p.esl) { const int rc = build_mip_bounds(c); if (rc) return rc; }

	uint32_t straddle = 1000u;
	if (c->tile_lane_map >= 0) { a.lane_map = (uint32_t) c->tile_lane_map; a.phase_x = c->tile_phase_x; a.phase_y = c->tile_phase_y; }
	else {
		vr_ctx::MipMap *hit = nullptr;
		for (uint32_t i = 0; i < c->mip_mapped && hit == nullptr; i++) {
			vr_ctx::MipMap &e = c->mip_map[i];
			if (memcmp(&e.p, p, sizeof *p) == 0 && memcmp(e.dim, c->dim, sizeof c->dim) == 0 && e.layout == a.layout && e.brick_plane == a.brick_plane) hit = &e;
		}
		if (hit == nullptr) {
			constexpr uint32_t kMaps = sizeof c->mip_map / sizeof c->mip_map[0];
			hit = &c->mip_map[c->mip_map_next];
			c->mip_map_next = (c->mip_map_next + 1) % kMaps;
			if (c->mip_mapped < kMaps) c->mip_mapped++;
			hit->straddle_permille = choose_tile_mapping(a);
			hit->p = *p; memcpy(hit->dim, c->dim, sizeof c->dim); hit->layout = a.layout; hit->brick_plane = a.brick_plane;
			hit->lane_map = a.lane_map; hit->phase_x = a.phase_x; hit->phase_y = a.phase_y;
		}
		a.lane_map = hit->lane_map; a.phase_x = hit->phase_x; a.phase_y = hit->phase_y; straddle = hit->straddle_permille;
	}
	const RaymarchPlan plan = plan_raymarch(a, brick_copy != nullptr, c->bpv);
	if (plan.reads_linear && c->vol == nullptr)
		return fail(c, VR_ERR_NOT_READY, (std::string("this ") + f.what + " frame needs the linear array, which was released (vr_hip_release_linear_copy): no resident brick copy "
		                                  "serves this sampling mode / addressing path — prepare it before releasing, or set the volume again").c_str());
	c->last_launch = vr_launch_info{ plan.reads_linear ? (uint32_t) kLayoutLinear : a.layout, a.brick_plane, a.lane_map, a.phase_x, a.phase_y, 0u, plan.tiles_x, plan.tiles_y, 0u, straddle, 0u, 0u, 0u };
	c->last_run_flavour = 0u;                    // (these frames read no run bricks)
	const uint8_t *bounds = a.p.esl ? c->mip_bounds : nullptr;
	if (f.leaping) { a.p.esl = params->esl; esl_divisor(a, params->esl_block_dims); transparent_corner_test(c, a); }
	uint64_t frame_seq = 0;
	return launch_timed(c, a, p, plan, brick_copy, stream, frame_seq, [&] { return launch(a, brick_copy, bounds); });
}

int launch_mip_frame(vr_ctx *c, const vr_params *p, void *dev_rgba, hipStream_t stream) {
	return launch_full_march_frame(c, p, stream, FullMarch{ "MIP", true, false, -1 }, [&](const RayKernelArgs &a, const void *brick_copy, const uint8_t *bounds) {
		return launch_mip(a, c->vol, brick_copy, c->bpv, c->tf, bounds, dev_rgba, stream);
	});
}

// One isosurface frame (include/vr_hip.h vr_hip_render_iso): what a MIP frame of the same view and sampling reads and maps, another kernel
int launch_iso_frame(vr_ctx *c, const vr_params *p, const vr_iso *iso, void *dev_rgba, void *dev_depth, hipStream_t stream) {
	return launch_full_march_frame(c, p, stream, FullMarch{ "isosurface", true, false, -1 }, [&](const RayKernelArgs &a, const void *brick_copy, const uint8_t *bounds) {
		return launch_iso(a, c->vol, brick_copy, c->bpv, c->tf, bounds, iso->level, iso->refine, dev_rgba, dev_depth, stream);
	});
}

// The light grid of a shadow (include/vr_hip.h vr_hip_set_shadow): S^3 bytes built by shadow_build_kernel from the copy full_march_copy gives
// a TRILINEAR frame of zeroed params on plane (x,y) — its quad bricks, the oct bricks for 2-byte voxels (no perspective, no pixel pitch: at
// most one cell per pixel), the linear array under VR_LAYOUT_LINEAR — on the context's stream, synchronous like a brick copy's first use.
// Waits for the context's frames first: one of them may still read the bytes it rewrites.
int build_shadow(vr_ctx *c) {
	if (c->shadow_ready) return VR_OK;
	const vr_shadow &sh = c->shadow;
	const uint64_t bytes = (uint64_t) sh.dims * sh.dims * sh.dims;
	VR_TRY(c, drain(c));
	if (c->shadow_q_bytes < bytes) {
		if (c->shadow_q) { (void) hipFree(c->shadow_q); c->shadow_q = nullptr; c->shadow_q_bytes = 0; }
		VR_TRY(c, hipMalloc((void **) &c->shadow_q, bytes));
		c->shadow_q_bytes = bytes;
	}
	vr_params p;
	memset(&p, 0, sizeof p);
	p.sampling = VR_SAMPLE_TRILINEAR;            // (the selector's row; the builder takes Q8 as a flag)
	RayKernelArgs a;
	volume_args(c, &p, a);
	const void *brick_copy = full_march_copy(c, &p, (int32_t) kPlaneXY, a);      // (always plane (x,y), whatever plane is forced on the frames)
	const RaymarchPlan plan = plan_raymarch(a, brick_copy != nullptr, c->bpv);
	if (plan.reads_linear && c->vol == nullptr)
		return fail(c, VR_ERR_NOT_READY, "the light grid of the shadow needs the linear array, which was released (vr_hip_release_linear_copy), and no resident brick copy serves it");
	ShadowBuildArgs s;
	memset(&s, 0, sizeof s);
	for (int i = 0; i < 3; i++) s.light[i] = sh.light_pos[i];
	s.dims = sh.dims; s.node_scale = 2.0f / (float) (sh.dims - 1u);
	s.step = sh.step; s.cutoff = sh.cutoff; s.q8 = sh.sampling == VR_SAMPLE_TRILINEAR_Q8 ? 1u : 0u;
	s.max_steps = (uint32_t) std::ceil(2.0 * std::sqrt(3.0) / (double) sh.step) + 2u;
	s.clip_on = c->clip_on ? 1u : 0u;
#ifdef VR_BOUNDS_CHECK
	VR_TRY(c, bounds_check_arm(c, a, &p, plan, brick_copy, 0u));
#endif
	VR_TRY(c, hipEventRecord(c->aux_start, c->stream));
	VR_TRY(c, launch_shadow_build(a, s, c->vol, brick_copy, c->bpv, c->tf, c->shadow_q, c->stream));
	VR_TRY(c, hipEventRecord(c->aux_stop, c->stream));
	VR_TRY(c, hipStreamSynchronize(c->stream));
#ifdef VR_BOUNDS_CHECK
	{ const int bc = bounds_check_verdict(c, c->stream, a.layout); if (bc) return bc; }
#endif
	(void) hipEventElapsedTime(&c->shadow_build_ms, c->aux_start, c->aux_stop);
	c->shadow_builds++;
	c->shadow_ready = true;
	return VR_OK;
}

// what the two isosurface entry points check beyond render_preamble
int validate_iso(vr_ctx *c, const vr_params *p, const vr_iso *iso) {
	if (iso == nullptr) return fail(c, VR_ERR_INVALID, "iso is NULL");
	if (const int rc = need_interpolated(c, p, "an isosurface")) return rc;
	if (!std::isfinite(iso->level)) return fail(c, VR_ERR_INVALID, "iso level must be finite");
	if (iso->refine > 16u) return fail(c, VR_ERR_INVALID, "iso refine must be in 0..16");
	return VR_OK;
}

// what the four render entry points check first; host_frame: the frame goes through the window buffer to host memory
int render_preamble(vr_ctx *c, const vr_params *p, const void *buffer, bool host_frame) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (buffer == nullptr) return fail(c, VR_ERR_INVALID, "buffer is NULL");      // GPURenderer1.cu:101-102
	int rc = validate_params(c, p);
	if (rc) return rc;
	rc = ready(c);
	if (rc) return rc;
	if (host_frame && (c->fb == nullptr || (size_t) p->out_width * p->out_rows * 4 > c->fb_bytes))
		return fail(c, VR_ERR_NOT_READY, "output larger than the window buffer: call vr_hip_set_window first");
	VR_TRY(c, hipSetDevice(c->device));
	return VR_OK;
}

// what the two backdrop entry points check beyond render_preamble
int validate_backdrop(vr_ctx *c, const vr_params *p, const vr_backdrop *bd) {
	if (bd == nullptr) return fail(c, VR_ERR_INVALID, "backdrop is NULL");
	if (bd->rgba == nullptr || bd->depth == nullptr) return fail(c, VR_ERR_INVALID, "backdrop rgba / depth is NULL");
	return need_interpolated(c, p, "a backdrop frame");
}

// a context-owned device buffer of at least `bytes`: allocated on first use and grown (behind the context's frames, one of which may
// still read the old one), never per frame
int grow_buffer(vr_ctx *c, void **buffer, size_t &have, size_t bytes) {
	if (have >= bytes) return VR_OK;
	VR_TRY(c, drain(c));
	if (*buffer) { (void) hipFree(*buffer); *buffer = nullptr; have = 0; }
	VR_TRY(c, hipMalloc(buffer, bytes));
	have = bytes;
	return VR_OK;
}

// The two composed forms (include/vr_hip.h: the hybrid, the section in the volume): first(depth buffer) renders its frame into dev_rgba and
// the depth buffer — the context's own when the caller gives none —, then the backdrop frame goes over it in place, on one stream
template <class First>
int launch_under_volume(vr_ctx *c, const vr_params *p, void *dev_rgba, void *dev_depth, hipStream_t stream, First &&first) {
	if (dev_depth == nullptr) {
		if (const int rc = grow_buffer(c, (void **) &c->hybrid_depth, c->hybrid_depth_bytes, (size_t) p->out_width * p->out_rows * sizeof(float))) return rc;
		dev_depth = c->hybrid_depth;
	}
	if (const int rc = first(dev_depth)) return rc;
	const vr_backdrop layer = { dev_rgba, dev_depth };
	return launch_frame(c, p, dev_rgba, stream, &layer);
}
int launch_hybrid(vr_ctx *c, const vr_params *p, const vr_iso *iso, void *dev_rgba, void *dev_depth, hipStream_t stream) {
	return launch_under_volume(c, p, dev_rgba, dev_depth, stream, [&](void *depth) { return launch_iso_frame(c, p, iso, dev_rgba, depth, stream); });
}

// what the four section entry points check beyond render_preamble (include/vr_hip.h, step 10 of the section contract)
int validate_section(vr_ctx *c, const vr_params *p, const vr_section *s) {
	if (s == nullptr) return fail(c, VR_ERR_INVALID, "section is NULL");
	if (const int rc = need_interpolated(c, p, "a section")) return rc;
	for (int i = 0; i < 4; i++)
		if (!std::isfinite(s->plane[i])) return fail(c, VR_ERR_INVALID, "section plane must be finite");
	if (!std::isfinite(s->half_width) || !std::isfinite(s->window[0]) || !std::isfinite(s->window[1]))
		return fail(c, VR_ERR_INVALID, "section half_width and window must be finite");
	if (s->plane[0] == 0.0f && s->plane[1] == 0.0f && s->plane[2] == 0.0f) return fail(c, VR_ERR_INVALID, "section normal is zero");
	if (s->mode > VR_SECTION_MEAN) return fail(c, VR_ERR_INVALID, "section mode must be in 0..3");
	if (s->half_width < 0.0f) return fail(c, VR_ERR_INVALID, "section half_width must not be negative");
	if (s->mode == VR_SECTION_POINT && s->half_width != 0.0f) return fail(c, VR_ERR_INVALID, "a POINT section has half_width 0");
	if (s->mode != VR_SECTION_POINT && s->half_width == 0.0f) return fail(c, VR_ERR_INVALID, "a thick section needs half_width > 0");
	if (!(s->window[0] == 0.0f && s->window[1] == 0.0f) && !(s->window[1] > s->window[0]))
		return fail(c, VR_ERR_INVALID, "section window must be {0, 0} or hi > lo");
	return VR_OK;
}

// One section frame (include/vr_hip.h vr_hip_render_section): what a clipped MIP frame of the same view and sampling reads and maps, without
// its block maxima (every sample is fetched), another kernel.  volume_args has filled the clip words, the identity clip when none is set.
int launch_section_frame(vr_ctx *c, const vr_params *p, const vr_section *s, void *dev_rgba, void *dev_depth, hipStream_t stream) {
	SectionArgs sa;
	memset(&sa, 0, sizeof sa);
	for (int i = 0; i < 4; i++) sa.plane[i] = s->plane[i];
	sa.half_width = s->half_width;
	sa.mode = s->mode;
	sa.windowed = (s->window[0] == 0.0f && s->window[1] == 0.0f) ? 0u : 1u;
	sa.window_lo = s->window[0];
	sa.window_inv = sa.windowed ? 1.0f / (s->window[1] - s->window[0]) : 0.0f;
	const int rc = launch_full_march_frame(c, p, stream, FullMarch{ "section", false, false, -1 }, [&](const RayKernelArgs &a, const void *brick_copy, const uint8_t *) {
		return launch_section(a, sa, c->vol, brick_copy, c->bpv, c->tf, dev_rgba, dev_depth, stream);
	});
	if (rc == VR_OK) c->section_frames++;
	return rc;
}

int launch_section_in_volume(vr_ctx *c, const vr_params *p, const vr_section *sec, void *dev_rgba, void *dev_depth, hipStream_t stream) {
	return launch_under_volume(c, p, dev_rgba, dev_depth, stream, [&](void *depth) { return launch_section_frame(c, p, sec, dev_rgba, depth, stream); });
}

// what the depth entry points check beyond render_preamble (include/vr_hip.h, step 10 of the depth contract)
int validate_depth(vr_ctx *c, const vr_params *p, const vr_depth *d) {
	if (d == nullptr) return fail(c, VR_ERR_INVALID, "depth is NULL");
	if (const int rc = need_interpolated(c, p, "a depth frame")) return rc;
	if (d->mode > VR_DEPTH_MEAN) return fail(c, VR_ERR_INVALID, "depth mode must be in 0..2");
	if (!std::isfinite(d->opacity) || d->opacity < 0.0f || d->opacity > 1.0f) return fail(c, VR_ERR_INVALID, "depth opacity must be finite and in [0, 1]");
	if (d->mode == VR_DEPTH_FIRST && d->opacity == 0.0f) return fail(c, VR_ERR_INVALID, "a FIRST depth needs opacity > 0: a transparent sample would be a surface");
	return VR_OK;
}

// One depth frame (include/vr_hip.h vr_hip_render_depth): what a clipped MIP frame of the same view and sampling reads and maps — no block
// maxima are built and the volume's own grid is not looked at —, with the composite's leaping (params.esl, the ESL bits of
// vr_hip_set_transfer_fn, the block grid of the params) and its transparent-sample test in the kernel argument (FullMarch::leaping), and the
// classification is the context's.  volume_args has filled the clip words.
int launch_depth_frame(vr_ctx *c, const vr_params *p, const vr_depth *d, const vr_depth_out *out, hipStream_t stream) {
	DepthArgs da;
	da.opacity = d->opacity; da.mode = d->mode; da.slab = c->preint_on ? 1u : 0u; da.want_alpha = out->alpha != nullptr ? 1u : 0u;
	const int rc = launch_full_march_frame(c, p, stream, FullMarch{ "depth", false, true, -1 }, [&](const RayKernelArgs &a, const void *brick_copy, const uint8_t *) {
		return launch_depth(a, da, c->vol, brick_copy, c->bpv, c->tf, c->esl, out->depth, out->value, out->alpha, stream);
	});
	if (rc == VR_OK) c->depth_frames++;
	return rc;
}

// the label table on the device: allocated on first use, the identity until vr_hip_set_label_table replaces it
int ensure_label_table(vr_ctx *c) {
	if (c->label_table != nullptr) return VR_OK;
	std::vector<float> identity(5u * VR_LABEL_COUNT, 0.0f);
	for (uint32_t i = 0; i < VR_LABEL_COUNT; i++) identity[5u * i + 4u] = 1.0f;
	VR_TRY(c, hipMalloc((void **) &c->label_table, identity.size() * sizeof(float)));
	VR_TRY(c, hipMemcpy(c->label_table, identity.data(), identity.size() * sizeof(float), hipMemcpyHostToDevice));
	return VR_OK;
}

// the labels in the 1-byte voxel-brick order (launch_brickify_voxel: the builder of the NEAREST copy, on the label array), on the context's
// stream and synchronous like a brick copy's first use; NULL where it cannot be had — the frame then reads the linear labels
const uint8_t *label_bricks_for(vr_ctx *c) {
	if (c->label_bricks != nullptr || c->label_bricks_failed) return c->label_bricks;
	uint8_t *dst = nullptr;
	const uint64_t bytes = bricked_elems(c->dim[0], c->dim[1], c->dim[2]);
	hipError_t e = hipMalloc((void **) &dst, bytes);
	if (e == hipSuccess) e = launch_brickify_voxel(c->labels, dst, 1u, c->dim[0], c->dim[1], c->dim[2], c->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
	if (e != hipSuccess) { (void) hipGetLastError(); if (dst) (void) hipFree(dst); c->label_bricks_failed = true; return nullptr; }
	c->label_bricks = dst;
	return dst;
}

// what the two labelled entry points check beyond render_preamble (include/vr_hip.h, step 11 of the label contract)
int validate_labelled(vr_ctx *c, const vr_params *p) {
	if (const int rc = need_interpolated(c, p, "a labelled frame")) return rc;
	if (c->preint_on)
		return fail(c, VR_ERR_INVALID, "pre-integration is set: a slab between two samples with different labels has no single table entry "
		                               "(vr_hip_set_preintegration(ctx, 0) switches it off)");
	if (c->labels == nullptr) return fail(c, VR_ERR_NOT_READY, "no labels are set for the resident volume (vr_hip_set_labels)");
	return VR_OK;
}

// One labelled frame (include/vr_hip.h vr_hip_render_labelled): what a depth frame of the same view and sampling reads and maps, with the
// composite's leaping and its transparent-sample test in the kernel argument, and the lighting and the shadow as launch_frame puts them
// there.  1-byte voxels read the (x,y) quad copy whatever the view (unless a plane is forced): the label bricks follow that order, and the
// kernel addresses them with the field's tables.  volume_args has filled the clip words.
int launch_labelled_frame(vr_ctx *c, const vr_params *p, void *dev_rgba, hipStream_t stream) {
	if (c->shadow_on) { if (const int rc = build_shadow(c)) return rc; }
	if (const int rc = ensure_label_table(c)) return rc;
	const FullMarch f = { "labelled", false, true, c->bpv == 1u && c->brick_plane_force < 0 ? (int32_t) kPlaneXY : -1 };
	const int rc = launch_full_march_frame(c, p, stream, f, [&](RayKernelArgs &a, const void *brick_copy, const uint8_t *) {
		lighting_shadow_args(c, a);
		const bool xy_quads = brick_copy != nullptr && c->bpv == 1u && a.layout == kLayoutBricked && a.brick_plane == kPlaneXY;
		return launch_labelled(a, c->labels, xy_quads ? label_bricks_for(c) : nullptr, c->vol, brick_copy, c->bpv, c->tf, c->esl, c->label_table, dev_rgba, stream);
	});
	if (rc == VR_OK) c->labelled_frames++;
	return rc;
}

// what the two tf2d entry points check beyond render_preamble (include/vr_hip.h, step 11 of the tf2d contract)
int validate_tf2d(vr_ctx *c, const vr_params *p) {
	if (const int rc = need_interpolated(c, p, "a tf2d frame")) return rc;
	if (c->preint_on)
		return fail(c, VR_ERR_INVALID, "pre-integration is set: a slab between two samples has no single row of the 2-D table "
		                               "(vr_hip_set_preintegration(ctx, 0) switches it off)");
	if (c->tf2d_table == nullptr) return fail(c, VR_ERR_NOT_READY, "no 2-D transfer function is set (vr_hip_set_tf2d)");
	return VR_OK;
}

// One tf2d frame (include/vr_hip.h vr_hip_render_tf2d): what a labelled frame of the same view and sampling reads and maps — the context's
// forced plane is left alone —, with the composite's leaping in the kernel argument, the lighting and the shadow as launch_frame puts them
// there, and tf_zero_below and the corner test of the table's ENVELOPE in this frame's copy of the arguments.  volume_args has filled the
// clip words.
int launch_tf2d_frame(vr_ctx *c, const vr_params *p, void *dev_rgba, hipStream_t stream) {
	if (c->shadow_on) { if (const int rc = build_shadow(c)) return rc; }
	const FullMarch f = { "tf2d", false, true, -1 };
	const int rc = launch_full_march_frame(c, p, stream, f, [&](RayKernelArgs &a, const void *brick_copy, const uint8_t *) {
		lighting_shadow_args(c, a);
		a.tf_zero_below = c->tf2d_zero_below;
		transparent_corner_test(c, a, c->tf2d_zero_below);
		Tf2dArgs d;
		d.g_scale = c->tf2d_g_scale; d.top = (float) (c->tf2d_rows - 1u); d.last = c->tf2d_rows - 2u; d.rows = c->tf2d_rows;
		for (int i = 0; i < 4; i++) d.g_dependent[i] = c->tf2d_g_dependent[i];
		return launch_tf2d(a, d, c->vol, brick_copy, c->bpv, c->tf2d_table, c->tf2d_esl, dev_rgba, stream);
	});
	if (rc == VR_OK) c->tf2d_frames++;
	return rc;
}

// Field B in the order of the copy a fused frame reads the resident volume in — layout kLayoutBricked on chunk plane `plane`, or kLayoutOct —:
// built from B's linear array by the builder of that copy (launch_brickify, launch_brickify_oct: free functions over a linear array), on the
// context's stream and synchronous like a brick copy's first use, under build_copy's rule that half of the HBM stays free; kept per kind
// until B goes.  NULL where it cannot be had: the frame then reads both linear arrays.  Testing aid: VR_SECOND_COPY_REFUSE=1 in the
// environment refuses every build as the HBM rule would (read at a copy's first use; a refusal holds until B is set again).
const void *second_copy_for(vr_ctx *c, uint32_t layout, uint32_t plane) {
	if (c->second == nullptr || (layout != kLayoutBricked && layout != kLayoutOct) || plane >= kPlanes || (layout == kLayoutOct && c->bpv != 2u)) return nullptr;
	const uint32_t slot = layout == kLayoutOct ? 3u : plane;
	if (c->second_copy[slot] != nullptr || c->second_copy_failed[slot]) return c->second_copy[slot];
	const uint64_t bytes = copy_bytes(c, layout == kLayoutOct ? (uint32_t) kCopyOct : kCopyQuadXY + plane);
	size_t free_b = 0, total_b = 0;
	void *dst = nullptr;
	hipError_t e = hipMemGetInfo(&free_b, &total_b);
	if (e == hipSuccess && (bytes >= free_b || free_b - bytes < total_b / 2)) e = hipErrorOutOfMemory;
	if (const char *refuse = getenv("VR_SECOND_COPY_REFUSE")) if (atoi(refuse) == 1) e = hipErrorOutOfMemory;
	if (e == hipSuccess) e = hipMalloc(&dst, bytes);
	if (e == hipSuccess) e = layout == kLayoutOct ? launch_brickify_oct(c->second, dst, c->dim[0], c->dim[1], c->dim[2], c->stream)
	                                              : launch_brickify(c->second, dst, c->bpv, plane, c->dim[0], c->dim[1], c->dim[2], c->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
	if (e != hipSuccess) { (void) hipGetLastError(); if (dst) (void) hipFree(dst); c->second_copy_failed[slot] = true; return nullptr; }
	c->second_copy[slot] = dst;
	return dst;
}

// what the two fused entry points check beyond render_preamble (include/vr_hip.h, step 13 of the fusion contract)
int validate_fused(vr_ctx *c, const vr_params *p, const vr_fusion *f) {
	if (f == nullptr) return fail(c, VR_ERR_INVALID, "fusion is NULL");
	if (const int rc = need_interpolated(c, p, "a fused frame")) return rc;
	if (f->mode > VR_FUSE_OVER) return fail(c, VR_ERR_INVALID, "fusion mode must be VR_FUSE_SUM or VR_FUSE_OVER");
	if (f->reserved != 0u) return fail(c, VR_ERR_INVALID, "fusion reserved must be 0");
	if (!std::isfinite(f->weight_a) || !std::isfinite(f->weight_b) || f->weight_a < 0.0f || f->weight_a > 1.0f || f->weight_b < 0.0f || f->weight_b > 1.0f)
		return fail(c, VR_ERR_INVALID, "fusion weights must be finite and in [0, 1]");
	if (c->preint_on)
		return fail(c, VR_ERR_INVALID, "pre-integration is set: a fused frame is defined per sample, not per slab (vr_hip_set_preintegration(ctx, 0) switches it off)");
	if (c->second == nullptr) return fail(c, VR_ERR_NOT_READY, "no second volume is set for the resident volume (vr_hip_set_second_volume)");
	if (c->second_tf == nullptr) return fail(c, VR_ERR_NOT_READY, "no transfer function is set for the second volume (vr_hip_set_second_transfer_fn)");
	return VR_OK;
}

// One fused frame (include/vr_hip.h vr_hip_render_fused): what a tf2d frame of the same view and sampling reads and maps — the context's forced
// plane is left alone —, with the composite's leaping on the fused frame's own bits in the kernel argument, the lighting and the shadow as
// launch_frame puts them there, and B's corner test and zero count beside A's.  B is read in the order the frame reads the resident volume
// in (FullMarch::second_field): where full_march_copy picks a brick copy and B's copy of that kind cannot be had, the frame is planned and
// launched as a VR_LAYOUT_LINEAR frame instead — both fields from their linear arrays.  volume_args has filled the clip words.
int launch_fused_frame(vr_ctx *c, const vr_params *p, const vr_fusion *fusion, void *dev_rgba, hipStream_t stream) {
	if (c->shadow_on) { if (const int rc = build_shadow(c)) return rc; }
	const FullMarch f = { "fused", false, true, -1, true };
	const int rc = launch_full_march_frame(c, p, stream, f, [&](RayKernelArgs &a, const void *brick_copy, const uint8_t *) {
		lighting_shadow_args(c, a);
		RayKernelArgs b = a;                         // B's corner test from B's own function: the same derivation on a scratch copy
		transparent_corner_test(c, b, c->second_zero_below);
		FusedArgs d;
		memset(&d, 0, sizeof d);
		d.weight_a = fusion->weight_a; d.weight_b = fusion->weight_b; d.mode = fusion->mode;
		d.skip_mask_b = b.skip_mask; d.skip_cmp_b = b.skip_cmp; d.tf_zero_below_b = c->second_zero_below;
		// (the copy is there: launch_full_march_frame planned a linear frame where it is not)
		return launch_fused(a, d, c->vol, brick_copy, c->second, brick_copy != nullptr ? second_copy_for(c, a.layout, a.brick_plane) : nullptr, c->bpv,
		                    c->tf, c->fused_esl, c->second_tf, dev_rgba, stream);
	});
	if (rc == VR_OK) c->fused_frames++;
	return rc;
}

// the depth buffer of the host entry points that hand a depth back (vr_hip_render_iso, vr_hip_render_section): one float per pixel of the
// window, sized with the window (render_preamble: the frame fits), allocated on first use behind the context's frames
int size_host_depth(vr_ctx *c) {
	if (c->iso_depth_bytes == c->fb_bytes) return VR_OK;
	VR_TRY(c, drain(c));
	if (c->iso_depth) { (void) hipFree(c->iso_depth); c->iso_depth = nullptr; c->iso_depth_bytes = 0; }
	VR_TRY(c, hipMalloc((void **) &c->iso_depth, c->fb_bytes));
	c->iso_depth_bytes = c->fb_bytes;
	return VR_OK;
}

// ... and what the two host-buffer ones end with: the frame in host memory (where the reference's timed region ends, GPURenderer1.cu:107-110)
// and the time since t0
void take_total_time(vr_ctx *c, std::chrono::steady_clock::time_point t0) {
	c->last_total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
	if (c->last_total_ms > c->total_ms_max) c->total_ms_max = c->last_total_ms;
}
int frame_to_host(vr_ctx *c, uint8_t *host_rgba, size_t bytes, std::chrono::steady_clock::time_point t0) {
	VR_TRY(c, hipMemcpyAsync(host_rgba, c->fb, bytes, hipMemcpyDeviceToHost, c->stream));
	VR_TRY(c, hipStreamSynchronize(c->stream));
	take_total_time(c, t0);
	return VR_OK;
}

// The two entry points of a feature frame (MIP, isosurface, hybrid, section, section in the volume, labelled), each written once: the
// preamble, what the feature checks beyond it (validate()), then the launch.  The device one: launch(stream) on the caller's stream or the
// context's.
template <class Validate, class Launch>
int render_to_device(vr_ctx *c, const vr_params *p, void *dev_rgba, void *stream, Validate &&validate, Launch &&launch) {
	if (const int rc = render_preamble(c, p, dev_rgba, false)) return rc;
	if (const int rc = validate()) return rc;
	return launch(stream ? (hipStream_t) stream : c->stream);
}
// The host one: launch(depth buffer) into the window buffer on the context's stream, timed until the frame is in host memory.  depth: the
// context's buffer the frame leaves its depth in, copied out where the caller gave host_depth — iso_depth, sized here before t0 and handed
// to the launch only then, or hybrid_depth, which the composed forms grow and use by themselves (the launch gets NULL) —, NULL = no depth.
template <class Validate, class Launch>
int render_to_host(vr_ctx *c, const vr_params *p, uint8_t *host_rgba, float *host_depth, float *vr_ctx::*depth, Validate &&validate, Launch &&launch) {
	int rc = render_preamble(c, p, host_rgba, true);
	if (rc) return rc;
	rc = validate();
	if (rc) return rc;
	const size_t pixels = (size_t) p->out_width * p->out_rows;
	const bool sized_here = host_depth != nullptr && depth == &vr_ctx::iso_depth;
	if (sized_here) { const int sized = size_host_depth(c); if (sized) return sized; }
	const auto t0 = std::chrono::steady_clock::now();
	rc = launch(sized_here ? c->iso_depth : nullptr);
	if (rc) return rc;
	if (host_depth != nullptr) VR_TRY(c, hipMemcpyAsync(host_depth, c->*depth, pixels * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	return frame_to_host(c, host_rgba, pixels * 4, t0);
}
const auto nothing_more = [] { return (int) VR_OK; };

// the six vr_hip_*_frames getters
int frames_counted(vr_ctx *c, uint64_t vr_ctx::*count, uint64_t *frames_out) {
	if (c == nullptr || frames_out == nullptr) return VR_ERR_INVALID;
	*frames_out = c->*count;
	return VR_OK;
}

}  // namespace

extern "C" {

const char *vr_hip_version(void) { return "vr_hip 0.1 (gfx950)"; }

int vr_hip_create(int device, vr_ctx **out) {
	if (out == nullptr) return VR_ERR_INVALID;
	*out = nullptr;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) {
		(void) hipGetLastError();
		return VR_ERR_NO_DEVICE;                 // no CPU fallback: the product path needs an MI355X
	}
	vr_ctx *c = new (std::nothrow) vr_ctx();
	if (c == nullptr) return VR_ERR_ALLOC;
	c->device = device;
	*out = c;                                    // handed out even on failure below so last_error stays readable
	VR_TRY(c, hipSetDevice(device));
	VR_TRY(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
	{
		int least = 0, greatest = 0;
		VR_TRY(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
		VR_TRY(c, hipStreamCreateWithPriority(&c->stream_first, hipStreamNonBlocking, greatest));
	}
	VR_TRY(c, hipMalloc((void **) &c->tf, 2 * VR_TF_SIZE * 4 * sizeof(float)));      // the 128 entries, and their running integral K behind them
	VR_TRY(c, hipMalloc((void **) &c->esl, VR_ESL_VOLUME_SIZE * sizeof(uint32_t)));
	VR_TRY(c, hipMalloc((void **) &c->minmax, 32 * 32 * 32 * 2));
	VR_TRY(c, hipMalloc((void **) &c->hist, 256 * sizeof(unsigned long long)));
	for (int i = 0; i < kEventRing; i++) {
		VR_TRY(c, hipEventCreate(&c->ring[i].start));
		VR_TRY(c, hipEventCreate(&c->ring[i].stop));
	}
	VR_TRY(c, hipEventCreate(&c->aux_start));
	VR_TRY(c, hipEventCreate(&c->aux_stop));
	return VR_OK;
}

void vr_hip_destroy(vr_ctx *c) {
	if (c == nullptr) return;
	(void) hipSetDevice(c->device);
	if (c->stream) (void) hipStreamSynchronize(c->stream);
	for (int i = 0; i < kEventRing; i++) {
		if (c->ring[i].start) (void) hipEventDestroy(c->ring[i].start);
		if (c->ring[i].stop) (void) hipEventDestroy(c->ring[i].stop);
	}
	if (c->aux_start) (void) hipEventDestroy(c->aux_start);
	if (c->aux_stop) (void) hipEventDestroy(c->aux_stop);
	if (c->cost_map) (void) hipFree(c->cost_map);
#ifdef VR_BOUNDS_CHECK
	if (c->bc_fault) (void) hipFree(c->bc_fault);
#endif
	for (auto &e : c->map_cache) { if (e.cost) (void) hipFree(e.cost); if (e.order) (void) hipFree(e.order); if (e.order_ready) (void) hipEventDestroy(e.order_ready); }
	for (auto &e : c->order_cache) for (auto &sl : e.slot) { if (sl.cost) (void) hipFree(sl.cost); if (sl.order) (void) hipFree(sl.order); if (sl.ready) (void) hipEventDestroy(sl.ready); }
	if (c->fb) (void) hipFree(c->fb);
	if (c->tf) (void) hipFree(c->tf);
	if (c->esl) (void) hipFree(c->esl);
	if (c->vol) (void) hipFree(c->vol);
	free_bricks(c);
	if (c->minmax) (void) hipFree(c->minmax);
	if (c->mip_bounds) (void) hipFree(c->mip_bounds);
	if (c->iso_depth) (void) hipFree(c->iso_depth);
	if (c->hybrid_depth) (void) hipFree(c->hybrid_depth);
	if (c->backdrop_stage) (void) hipFree(c->backdrop_stage);
	if (c->depth_stage) (void) hipFree(c->depth_stage);
	if (c->pick_stage) (void) hipFree(c->pick_stage);
	drop_labels(c);
	if (c->label_table) (void) hipFree(c->label_table);
	if (c->tf2d_table) (void) hipFree(c->tf2d_table);
	if (c->tf2d_esl) (void) hipFree(c->tf2d_esl);
	drop_second(c);
	if (c->second_tf) (void) hipFree(c->second_tf);
	if (c->fused_esl) (void) hipFree(c->fused_esl);
	if (c->gradient_hist) (void) hipFree(c->gradient_hist);
	if (c->shadow_q) (void) hipFree(c->shadow_q);
	if (c->hist) (void) hipFree(c->hist);
	if (c->stream_first) { (void) hipStreamSynchronize(c->stream_first); (void) hipStreamDestroy(c->stream_first); }
	if (c->stream) (void) hipStreamDestroy(c->stream);
	delete c;
}

const char *vr_hip_last_error(const vr_ctx *c) { return c ? c->err.c_str() : "no context"; }

int vr_hip_set_window(vr_ctx *c, uint32_t w, uint32_t h) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (w == 0 || h == 0 || w > 65535u || h > 65535u) return fail(c, VR_ERR_INVALID, "window dims out of range (1..65535)");
	VR_TRY(c, hipSetDevice(c->device));
	const size_t bytes = (size_t) w * h * 4;
	if (bytes != c->fb_bytes) {
		if (c->fb) { (void) hipFree(c->fb); c->fb = nullptr; c->fb_bytes = 0; }
		VR_TRY(c, hipMalloc(&c->fb, bytes));
		c->fb_bytes = bytes;
	}
	c->win_w = w; c->win_h = h;
	return VR_OK;
}

int vr_hip_set_transfer_fn(vr_ctx *c, const float *tf, const uint32_t *esl) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (tf == nullptr || esl == nullptr) return fail(c, VR_ERR_INVALID, "transfer_fn / esl_volume is NULL");
	VR_TRY(c, hipSetDevice(c->device));
	// Frames queued by vr_hip_render_device run asynchronously (context stream or a caller's stream): wait for THIS CONTEXT'S
	// frames (the event ring records every one of them) before the tables they read are rewritten, then upload on the context
	// stream and wait again — the reference is synchronous here too, and calls this on every mouse-motion event of its TF editor
	// (UI.cpp:52-61,317-341), so other contexts and streams of the device are not stalled (no hipDeviceSynchronize).
	VR_TRY(c, drain(c));
	VR_TRY(c, hipMemcpyAsync(c->tf, tf, VR_TF_SIZE * 4 * sizeof(float), hipMemcpyHostToDevice, c->stream));
	// K, the running integral of the piecewise-linear transfer function (vr_hip_set_preintegration): K[0] = 0, K[i + 1] = fma(0.5, tf[i] + tf[i + 1], K[i])
	float integral[VR_TF_SIZE * 4];
	for (int ch = 0; ch < 4; ch++) {
		integral[ch] = 0.0f;
		for (int i = 0; i + 1 < VR_TF_SIZE; i++) integral[4 * (i + 1) + ch] = std::fmaf(0.5f, tf[4 * i + ch] + tf[4 * (i + 1) + ch], integral[4 * i + ch]);
	}
	VR_TRY(c, hipMemcpyAsync(c->tf + VR_TF_SIZE * 4, integral, sizeof integral, hipMemcpyHostToDevice, c->stream));      // (the stream is synchronised below, while `integral` lives)
	VR_TRY(c, hipMemcpyAsync(c->esl, esl, VR_ESL_VOLUME_SIZE * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	VR_TRY(c, hipStreamSynchronize(c->stream));
	int zero = -1;
	while (zero + 1 < VR_TF_SIZE && tf[4 * (zero + 1)] == 0.0f && tf[4 * (zero + 1) + 1] == 0.0f && tf[4 * (zero + 1) + 2] == 0.0f &&
	       tf[4 * (zero + 1) + 3] == 0.0f)
		zero++;
	c->tf_zero_below = (float) zero;
	c->tf_set = true;
	c->shadow_ready = false;                     // the light grid holds transmittances under the old transfer function
	forget_recorded_orders(c);                   // they describe ray lengths under the old transfer function (placement only; nothing is in flight here: drained above)
	return VR_OK;
}

int vr_hip_set_volume(vr_ctx *c, const void *host, uint32_t x, uint32_t y, uint32_t z, uint32_t bpv) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (host == nullptr) return fail(c, VR_ERR_INVALID, "volume data is NULL");     // GPURenderer1.cu:91-92
	VR_TRY(c, hipSetDevice(c->device));
	int rc = alloc_volume(c, x, y, z, bpv);
	if (rc) return rc;
	const auto t0 = std::chrono::steady_clock::now();
	VR_TRY(c, hipMemcpy(c->vol, host, c->vol_elems * bpv, hipMemcpyHostToDevice));
	VR_TRY(c, hipStreamSynchronize(c->stream));
	c->upload_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
	return VR_OK;                                // brick copies are built by the first frame that reads them (or vr_hip_prepare)
}

int vr_hip_set_volume_device(vr_ctx *c, const void *dev, uint32_t x, uint32_t y, uint32_t z, uint32_t bpv) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (dev == nullptr) return fail(c, VR_ERR_INVALID, "volume data is NULL");
	VR_TRY(c, hipSetDevice(c->device));
	int rc = alloc_volume(c, x, y, z, bpv);
	if (rc) return rc;
	// on the context's own (non-blocking) stream: a device-to-device hipMemcpy on the null stream may return before it has
	// finished and would not be ordered before the brick builder below
	const auto t0 = std::chrono::steady_clock::now();
	VR_TRY(c, hipMemcpyAsync(c->vol, dev, c->vol_elems * bpv, hipMemcpyDeviceToDevice, c->stream));
	VR_TRY(c, hipStreamSynchronize(c->stream));
	c->upload_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
	return VR_OK;
}

int vr_hip_set_layout(vr_ctx *c, uint32_t layout) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (layout != VR_LAYOUT_LINEAR && layout != VR_LAYOUT_BRICKED) return fail(c, VR_ERR_INVALID, "unknown volume layout");
	VR_TRY(c, hipSetDevice(c->device));
	VR_TRY(c, drain(c));                         // a frame may still be reading the copies we are about to drop
	if (const int rc = need_linear(c, "the brick copies cannot be rebuilt or dropped")) return rc;
	c->layout = layout;
	free_bricks(c);
	forget_tile_mappings(c);
	return VR_OK;
}

int vr_hip_set_wide_addressing(vr_ctx *c, uint32_t force) {
	if (c == nullptr) return VR_ERR_INVALID;
	// The index-arithmetic path (1) reads the linear array for NEAREST: refused once that array was released (the frame
	// would otherwise be launched with a NULL volume pointer).  launch_frame checks the same for every frame.
	if ((force & 3u) == 1u) if (const int rc = need_linear(c, "the index-arithmetic path needs it")) return rc;
	c->force_wide = force & 3u;                  // 0 auto, 1 arithmetic 64-bit path, 2 table path with 64-bit z offsets
	c->force_clamp_fetch = (force >> 2) & 3u;    // + 4: clamp the fetch coordinates of every sample (far-away views do that);
	                                             // + 8: NEAREST never marches in the scaled domain (volumes with power-of-two edges do)
	return VR_OK;
}

int vr_hip_set_brick_plane(vr_ctx *c, int32_t plane) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (plane == (int32_t) kPlanes + 5 || plane == (int32_t) kPlanes + 6) {      // 8 / 9: the column windows for every orthogonal full-march frame / never
		c->column_force = plane == (int32_t) kPlanes + 5 ? 1 : -1;
		c->oct_always = false; c->brick_plane_force = -1;
		forget_tile_mappings(c);
		return VR_OK;
	}
	c->column_force = 0;
	if (plane < -1 || plane > (int32_t) kPlanes + 4)
		return fail(c, VR_ERR_INVALID, "plane must be -1 (per view), 0 (x,y), 1 (x,z), 2 (y,z), 3 (run bricks along z), 4 (run bricks along y), 5 (oct bricks for every view of a "
		                               "2-byte volume), 6 (both run copies, chosen per tile by measurement, for every full-march view), 7 (both run copies on alternating tiles), "
		                               "8 (column windows for every orthogonal full-march frame) or 9 (never the column windows)");
	c->oct_always = plane == (int32_t) kPlanes + 2;
	c->brick_plane_force = c->oct_always ? -1 : plane;
	forget_tile_mappings(c);                     // cached lane orders were chosen for another plane
	return VR_OK;
}

int vr_hip_set_column_copy(vr_ctx *c, uint32_t mode) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (mode > 2u) return fail(c, VR_ERR_INVALID, "column copy must be 0 (voxel windows where a wave's columns fit, else quad-element windows; lit frames shade from the "
	                                              "quad-element windows), 1 (quad-element windows) or 2 (as 0, shading from the voxel windows)");
	c->column_copy = mode;
	return VR_OK;
}

int vr_hip_set_run_flavour(vr_ctx *c, uint32_t flavour) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (flavour > 2u) return fail(c, VR_ERR_INVALID, "run flavour must be 0 (automatic), 1 (nine-element runs) or 2 (seven-cell aligned runs for full-march frames)");
	c->run_flavour = flavour;
	return VR_OK;
}

int vr_hip_run_aligned_info(vr_ctx *c, vr_run_aligned_info *out) {
	if (c == nullptr || out == nullptr) return VR_ERR_INVALID;
	memset(out, 0, sizeof *out);
	out->flavour = c->run_flavour; out->last_flavour = c->last_run_flavour;
	for (uint32_t k = kCopyRun7Z; k <= kCopyRun7Y; k++) {
		out->build_ms[k - kCopyRun7Z] = c->copy_build_ms[k];
		if (c->copy_failed[k]) out->copies_refused |= 1u << k;
		if (c->copy[k]) { out->copies |= 1u << k; out->bytes += copy_bytes(c, k); }
	}
	return VR_OK;
}

int vr_hip_set_tile_scheduling(vr_ctx *c, uint32_t mode) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (mode > 2u) return fail(c, VR_ERR_INVALID, "tile scheduling mode must be 0 (workgroup id), 1 (measured-cost order) or 2 (workgroup id + cost map)");
	c->tile_scheduling = mode;
	forget_recorded_orders(c);
	return VR_OK;
}

int vr_hip_set_clip(vr_ctx *c, const vr_clip *clip) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (clip != nullptr) {
		if (!finite3(clip->box_min) || !finite3(clip->box_max) || !finite3(clip->plane) || !std::isfinite(clip->plane[3]))
			return fail(c, VR_ERR_INVALID, "clip members must be finite");
		for (int i = 0; i < 3; i++)
			if (clip->box_min[i] >= clip->box_max[i]) return fail(c, VR_ERR_INVALID, "clip box_min must be below box_max on every axis");
	}
	const bool on = clip != nullptr;
	if (on == c->clip_on && (!on || memcmp(&c->clip, clip, sizeof *clip) == 0)) return VR_OK;
	// The mapping and order caches are keyed by vr_params alone.  Both are placement only — an order recorded under another clip would still
	// give the same image — but it describes other ray lengths and must not be mistaken for this clip's.  (Buffers of frames in flight stay.)
	c->clip_on = on;
	if (on) c->clip = *clip;
	c->shadow_ready = false;                     // light rays are clipped too
	forget_tile_mappings(c);
	forget_recorded_orders(c);
	return VR_OK;
}

int vr_hip_set_shadow(vr_ctx *c, const vr_shadow *sh) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (sh != nullptr) {
		if (!finite3(sh->light_pos) || !std::isfinite(sh->step) || !std::isfinite(sh->strength) || !std::isfinite(sh->cutoff))
			return fail(c, VR_ERR_INVALID, "shadow members must be finite");
		if (sh->dims < 2u || sh->dims > 256u) return fail(c, VR_ERR_INVALID, "shadow dims must be in 2..256");
		if (!(sh->step >= 1.0f / 4096.0f)) return fail(c, VR_ERR_INVALID, "shadow step must be >= 1/4096");
		if (!(sh->strength >= 0.0f && sh->strength <= 1.0f)) return fail(c, VR_ERR_INVALID, "shadow strength must be in 0..1");
		if (!(sh->cutoff >= 0.0f && sh->cutoff < 1.0f)) return fail(c, VR_ERR_INVALID, "shadow cutoff must be in [0, 1)");
		if (sh->sampling != VR_SAMPLE_TRILINEAR && sh->sampling != VR_SAMPLE_TRILINEAR_Q8)
			return fail(c, VR_ERR_INVALID, "shadow sampling must be VR_SAMPLE_TRILINEAR or VR_SAMPLE_TRILINEAR_Q8");
	}
	const bool on = sh != nullptr;
	if (on == c->shadow_on && (!on || memcmp(&c->shadow, sh, sizeof *sh) == 0)) return VR_OK;      // the same shadow: the light grid stays
	if (on && c->shadow_on) {                    // the strength alone: the grid does not depend on it, and the frames read the same copies
		vr_shadow same_grid = *sh;
		same_grid.strength = c->shadow.strength;
		if (memcmp(&c->shadow, &same_grid, sizeof same_grid) == 0) { c->shadow.strength = sh->strength; return VR_OK; }
	}
	c->shadow_on = on;
	if (on) c->shadow = *sh;
	c->shadow_ready = false;
	forget_tile_mappings(c);                     // as for a clip: the caches are keyed by vr_params alone, and a shadowed frame reads other copies
	forget_recorded_orders(c);
	return VR_OK;
}

int vr_hip_set_lighting(vr_ctx *c, const vr_lighting *l) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (l != nullptr) {
		if (!std::isfinite(l->ambient) || !std::isfinite(l->diffuse) || !std::isfinite(l->specular))
			return fail(c, VR_ERR_INVALID, "lighting members must be finite");
		if (!(l->ambient >= 0.0f && l->ambient <= 1.0f) || !(l->diffuse >= 0.0f && l->diffuse <= 1.0f) || !(l->specular >= 0.0f && l->specular <= 1.0f))
			return fail(c, VR_ERR_INVALID, "lighting ambient, diffuse and specular must be in 0..1");
		if (l->shininess_log2 > 10u) return fail(c, VR_ERR_INVALID, "lighting shininess_log2 must be in 0..10");
	}
	const bool on = l != nullptr;
	if (on == c->lighting_on && (!on || memcmp(&c->lighting, l, sizeof *l) == 0)) return VR_OK;
	c->lighting_on = on;
	if (on) c->lighting = *l;
	forget_tile_mappings(c);                     // as for a shadow: the caches are keyed by vr_params alone, and a lit frame reads other copies
	forget_recorded_orders(c);
	return VR_OK;
}

int vr_hip_lighting_frames(vr_ctx *c, uint64_t *frames_out) { return frames_counted(c, &vr_ctx::lit_frames, frames_out); }

int vr_hip_set_preintegration(vr_ctx *c, uint32_t on) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (on > 1u) return fail(c, VR_ERR_INVALID, "pre-integration must be 0 (off) or 1 (slab classification)");
	if ((on != 0u) == c->preint_on) return VR_OK;
	c->preint_on = on != 0u;
	forget_tile_mappings(c);                     // as for a lighting: the caches are keyed by vr_params alone, and a slab frame reads other copies
	forget_recorded_orders(c);
	return VR_OK;
}

int vr_hip_preint_frames(vr_ctx *c, uint64_t *frames_out) { return frames_counted(c, &vr_ctx::preint_frames, frames_out); }

int vr_hip_download_tf_integral(vr_ctx *c, float *host_out512) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (host_out512 == nullptr) return fail(c, VR_ERR_INVALID, "host_out512 is NULL");
	if (!c->tf_set) return fail(c, VR_ERR_NOT_READY, "no transfer function is set (vr_hip_set_transfer_fn)");
	VR_TRY(c, hipSetDevice(c->device));
	VR_TRY(c, hipMemcpy(host_out512, c->tf + VR_TF_SIZE * 4, VR_TF_SIZE * 4 * sizeof(float), hipMemcpyDeviceToHost));
	return VR_OK;
}

int vr_hip_download_shadow(vr_ctx *c, uint8_t *host_out, uint64_t capacity, uint32_t *dims_out) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (!c->shadow_on) return fail(c, VR_ERR_NOT_READY, "no shadow is set (vr_hip_set_shadow)");
	if (const int rc = ready(c)) return rc;
	const uint64_t bytes = (uint64_t) c->shadow.dims * c->shadow.dims * c->shadow.dims;
	if (dims_out) *dims_out = c->shadow.dims;
	if (host_out == nullptr && capacity == 0) return VR_OK;      // size query: only *dims_out
	if (host_out == nullptr || capacity < bytes) return fail(c, VR_ERR_INVALID, "shadow buffer is NULL or smaller than dims^3 bytes");
	VR_TRY(c, hipSetDevice(c->device));
	if (const int rc = build_shadow(c)) return rc;
	VR_TRY(c, hipMemcpyAsync(host_out, c->shadow_q, bytes, hipMemcpyDeviceToHost, c->stream));
	VR_TRY(c, hipStreamSynchronize(c->stream));
	return VR_OK;
}

int vr_hip_shadow_builds(vr_ctx *c, uint64_t *builds_out, float *last_build_ms_out) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (builds_out) *builds_out = c->shadow_builds;
	if (last_build_ms_out) *last_build_ms_out = c->shadow_build_ms;
	return VR_OK;
}

int vr_hip_last_launch(vr_ctx *c, vr_launch_info *out) {
	if (c == nullptr || out == nullptr) return VR_ERR_INVALID;
	*out = c->last_launch;
	return VR_OK;
}

int vr_hip_read_tile_costs(vr_ctx *c, uint32_t *host_out, uint32_t capacity, uint32_t *tiles_x, uint32_t *tiles_y) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (tiles_x) *tiles_x = c->cost_map_tiles_x;
	if (tiles_y) *tiles_y = c->cost_map_tiles_y;
	const uint32_t n = c->cost_map_tiles_x * c->cost_map_tiles_y;
	if (c->cost_map == nullptr || n == 0) return fail(c, VR_ERR_NOT_READY, "no cost map: render a frame with vr_hip_set_tile_scheduling(ctx, 2) first");
	if (host_out == nullptr) return VR_OK;                   // size query
	if (capacity < n) return fail(c, VR_ERR_INVALID, "cost map buffer too small");
	VR_TRY(c, hipSetDevice(c->device));
	VR_TRY(c, drain(c));
	std::vector<uint32_t> by_number(n);
	VR_TRY(c, hipMemcpy(by_number.data(), c->cost_map, (size_t) n * 4, hipMemcpyDeviceToHost));
	for (uint32_t t = 0; t < n; t++) {                        // tile number (blocks of tiles) -> row-major
		uint32_t x = 0, y = 0;
		tile_number_to_xy(t, c->cost_map_tiles_x, c->cost_map_tiles_y, &x, &y);
		host_out[(size_t) y * c->cost_map_tiles_x + x] = by_number[t];
	}
	return VR_OK;
}

int vr_hip_set_tile_mapping(vr_ctx *c, int32_t lane_map, uint32_t phase_x, uint32_t phase_y) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (lane_map < -1 || (lane_map >= 0 && ((lane_map & 3) > (int32_t) kLaneBlocks || (lane_map >> 2) > 2)) || phase_x > 7u || phase_y > 7u)
		return fail(c, VR_ERR_INVALID, "lane_map must be -1 or (order 0..2) + 4 * (wave shape 0..2), and the phases 0..7");
	c->tile_lane_map = lane_map; c->tile_phase_x = phase_x; c->tile_phase_y = phase_y;
	return VR_OK;
}

int vr_hip_render_device(vr_ctx *c, const vr_params *p, void *dev_rgba, void *stream) {
	if (const int rc = render_preamble(c, p, dev_rgba, false)) return rc;
	return launch_frame(c, p, dev_rgba, stream ? (hipStream_t) stream : c->stream);
}

int vr_hip_render(vr_ctx *c, const vr_params *p, uint8_t *host_rgba) {
	int rc = render_preamble(c, p, host_rgba, true);
	if (rc) return rc;
	const size_t bytes = (size_t) p->out_width * p->out_rows * 4;
	const auto t0 = std::chrono::steady_clock::now();
	// The reference's timed region ends with the frame in HOST memory (GPURenderer1.cu:107-110).  A frame of unpartitioned rows is
	// rendered as TWO row slices: the first on a stream of the highest priority, so that its workgroups are dispatched ahead of the
	// second slice's and it finishes about halfway through the frame; its copy to the host then runs while the second slice still
	// renders, and only the second half of the PCIe transfer is left behind the kernels (measured on the prototype,
	// scripts/host_slices_probe.py, C4: 2.32 ms per frame against 2.48 as one launch + one copy, the kernel alone 2.28 wall).  The
	// pixels are the same: a slice is a band partition (x0 / band fields of vr_params), the partition the multi-GPU path renders.
	static const int host_slices = [] { const char *e = getenv("VR_HOST_SLICES"); return e ? atoi(e) : 2; }();         // VR_HOST_SLICES=1: one launch + one copy (A/B)
	const uint32_t first_rows = ((p->out_rows + 1u) / 2u + 15u) & ~15u;      // whole workgroup tiles (32x16 pixels)
	if (host_slices >= 2 && p->band_stride == 1 && p->band_first == 0 && first_rows < p->out_rows && bytes >= (1u << 20)) {
		vr_params q = *p;
		q.band_rows = first_rows; q.band_stride = 2;                        // gy = band_first * first_rows + ly for ly < first_rows
		q.band_first = 0; q.out_rows = first_rows;
		rc = launch_frame(c, &q, c->fb, c->stream_first);
		if (rc) return rc;
		const size_t first_bytes = (size_t) first_rows * p->out_width * 4;
		q.band_first = 1; q.out_rows = p->out_rows - first_rows;
		rc = launch_frame(c, &q, (uint8_t *) c->fb + first_bytes, c->stream);
		if (rc) { (void) hipStreamSynchronize(c->stream_first); return rc; }
		VR_TRY(c, hipMemcpyAsync(host_rgba, c->fb, first_bytes, hipMemcpyDeviceToHost, c->stream_first));
		VR_TRY(c, hipMemcpyAsync(host_rgba + first_bytes, (uint8_t *) c->fb + first_bytes, bytes - first_bytes, hipMemcpyDeviceToHost, c->stream));
		VR_TRY(c, hipStreamSynchronize(c->stream_first));
		VR_TRY(c, hipStreamSynchronize(c->stream));
		take_total_time(c, t0);
		return VR_OK;
	}
	rc = launch_frame(c, p, c->fb, c->stream);
	if (rc) return rc;
	return frame_to_host(c, host_rgba, bytes, t0);
}

int vr_hip_render_mip_device(vr_ctx *c, const vr_params *p, void *dev_rgba, void *stream) {
	return render_to_device(c, p, dev_rgba, stream, nothing_more, [&](hipStream_t on) { return launch_mip_frame(c, p, dev_rgba, on); });
}

int vr_hip_render_mip(vr_ctx *c, const vr_params *p, uint8_t *host_rgba) {
	return render_to_host(c, p, host_rgba, nullptr, nullptr, nothing_more, [&](void *) { return launch_mip_frame(c, p, c->fb, c->stream); });
}

int vr_hip_render_iso_device(vr_ctx *c, const vr_params *p, const vr_iso *iso, void *dev_rgba, void *dev_depth, void *stream) {
	return render_to_device(c, p, dev_rgba, stream, [&] { return validate_iso(c, p, iso); }, [&](hipStream_t on) { return launch_iso_frame(c, p, iso, dev_rgba, dev_depth, on); });
}

int vr_hip_render_iso(vr_ctx *c, const vr_params *p, const vr_iso *iso, uint8_t *host_rgba, float *host_depth) {
	return render_to_host(c, p, host_rgba, host_depth, &vr_ctx::iso_depth, [&] { return validate_iso(c, p, iso); },
	                      [&](void *depth) { return launch_iso_frame(c, p, iso, c->fb, depth, c->stream); });
}

// ---- backdrop and hybrid frames (include/vr_hip.h vr_backdrop) ----

int vr_hip_render_backdrop_device(vr_ctx *c, const vr_params *p, const vr_backdrop *dev, void *dev_rgba, void *stream) {
	if (const int rc = render_preamble(c, p, dev_rgba, false)) return rc;
	if (const int rc = validate_backdrop(c, p, dev)) return rc;
	return launch_frame(c, p, dev_rgba, stream ? (hipStream_t) stream : c->stream, dev);
}

int vr_hip_render_backdrop(vr_ctx *c, const vr_params *p, const vr_backdrop *host, uint8_t *host_rgba) {
	int rc = render_preamble(c, p, host_rgba, true);
	if (rc) return rc;
	rc = validate_backdrop(c, p, host);
	if (rc) return rc;
	// the two layers are two caller-owned arrays: one upload each (one upload of both would need a host copy of our own first) into ONE
	// context-owned staging buffer, colour first, on the frame's stream
	const size_t pixels = (size_t) p->out_width * p->out_rows;
	if (const int grow = grow_buffer(c, &c->backdrop_stage, c->backdrop_stage_bytes, pixels * 8)) return grow;
	const auto t0 = std::chrono::steady_clock::now();
	VR_TRY(c, hipMemcpyAsync(c->backdrop_stage, host->rgba, pixels * 4, hipMemcpyHostToDevice, c->stream));
	VR_TRY(c, hipMemcpyAsync((uint8_t *) c->backdrop_stage + pixels * 4, host->depth, pixels * 4, hipMemcpyHostToDevice, c->stream));
	const vr_backdrop dev = { c->backdrop_stage, (uint8_t *) c->backdrop_stage + pixels * 4 };
	rc = launch_frame(c, p, c->fb, c->stream, &dev);
	if (rc) return rc;
	return frame_to_host(c, host_rgba, pixels * 4, t0);
}

int vr_hip_render_hybrid_device(vr_ctx *c, const vr_params *p, const vr_iso *iso, void *dev_rgba, void *dev_depth, void *stream) {
	return render_to_device(c, p, dev_rgba, stream, [&] { return validate_iso(c, p, iso); }, [&](hipStream_t on) { return launch_hybrid(c, p, iso, dev_rgba, dev_depth, on); });
}

int vr_hip_render_hybrid(vr_ctx *c, const vr_params *p, const vr_iso *iso, uint8_t *host_rgba, float *host_depth) {
	return render_to_host(c, p, host_rgba, host_depth, &vr_ctx::hybrid_depth, [&] { return validate_iso(c, p, iso); },
	                      [&](void *depth) { return launch_hybrid(c, p, iso, c->fb, depth, c->stream); });
}

int vr_hip_backdrop_frames(vr_ctx *c, uint64_t *frames_out) { return frames_counted(c, &vr_ctx::backdrop_frames, frames_out); }

// ---- section frames (include/vr_hip.h vr_section) ----

int vr_hip_render_section_device(vr_ctx *c, const vr_params *p, const vr_section *s, void *dev_rgba, void *dev_depth, void *stream) {
	return render_to_device(c, p, dev_rgba, stream, [&] { return validate_section(c, p, s); }, [&](hipStream_t on) { return launch_section_frame(c, p, s, dev_rgba, dev_depth, on); });
}

int vr_hip_render_section(vr_ctx *c, const vr_params *p, const vr_section *s, uint8_t *host_rgba, float *host_depth) {
	return render_to_host(c, p, host_rgba, host_depth, &vr_ctx::iso_depth, [&] { return validate_section(c, p, s); },
	                      [&](void *depth) { return launch_section_frame(c, p, s, c->fb, depth, c->stream); });
}

int vr_hip_render_section_in_volume_device(vr_ctx *c, const vr_params *p, const vr_section *s, void *dev_rgba, void *dev_depth, void *stream) {
	return render_to_device(c, p, dev_rgba, stream, [&] { return validate_section(c, p, s); }, [&](hipStream_t on) { return launch_section_in_volume(c, p, s, dev_rgba, dev_depth, on); });
}

int vr_hip_render_section_in_volume(vr_ctx *c, const vr_params *p, const vr_section *s, uint8_t *host_rgba, float *host_depth) {
	return render_to_host(c, p, host_rgba, host_depth, &vr_ctx::hybrid_depth, [&] { return validate_section(c, p, s); },
	                      [&](void *depth) { return launch_section_in_volume(c, p, s, c->fb, depth, c->stream); });
}

int vr_hip_section_frames(vr_ctx *c, uint64_t *frames_out) { return frames_counted(c, &vr_ctx::section_frames, frames_out); }

// ---- depth frames of the composite and picking (include/vr_hip.h vr_depth) ----

int vr_hip_render_depth_device(vr_ctx *c, const vr_params *p, const vr_depth *d, const vr_depth_out *dev, void *stream) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (dev == nullptr) return fail(c, VR_ERR_INVALID, "depth_out is NULL");
	if (const int rc = render_preamble(c, p, dev->depth, false)) return rc;
	if (const int rc = validate_depth(c, p, d)) return rc;
	return launch_depth_frame(c, p, d, dev, stream ? (hipStream_t) stream : c->stream);
}

int vr_hip_render_depth(vr_ctx *c, const vr_params *p, const vr_depth *d, const vr_depth_out *host) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (host == nullptr) return fail(c, VR_ERR_INVALID, "depth_out is NULL");
	int rc = render_preamble(c, p, host->depth, false);
	if (rc) return rc;
	rc = validate_depth(c, p, d);
	if (rc) return rc;
	// one launch, and one copy back per buffer asked for, out of one context-owned staging buffer: depth, value, alpha
	const size_t bytes = (size_t) p->out_width * p->out_rows * sizeof(float);
	if (const int grow = grow_buffer(c, &c->depth_stage, c->depth_stage_bytes, 3 * bytes)) return grow;
	uint8_t *stage = (uint8_t *) c->depth_stage;
	const vr_depth_out dev = { stage, host->value ? stage + bytes : nullptr, host->alpha ? stage + 2 * bytes : nullptr };
	const auto t0 = std::chrono::steady_clock::now();
	rc = launch_depth_frame(c, p, d, &dev, c->stream);
	if (rc) return rc;
	VR_TRY(c, hipMemcpyAsync(host->depth, dev.depth, bytes, hipMemcpyDeviceToHost, c->stream));
	if (host->value) VR_TRY(c, hipMemcpyAsync(host->value, dev.value, bytes, hipMemcpyDeviceToHost, c->stream));
	if (host->alpha) VR_TRY(c, hipMemcpyAsync(host->alpha, dev.alpha, bytes, hipMemcpyDeviceToHost, c->stream));
	VR_TRY(c, hipStreamSynchronize(c->stream));
	take_total_time(c, t0);
	return VR_OK;
}

int vr_hip_pick(vr_ctx *c, const vr_params *p, const vr_depth *d, uint32_t n, const uint32_t *xy, vr_pick *out) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (n == 0u) return VR_OK;
	if (n > VR_PICK_MAX) return fail(c, VR_ERR_INVALID, "at most VR_PICK_MAX (256) pixels per pick");
	if (xy == nullptr) return fail(c, VR_ERR_INVALID, "xy is NULL");
	int rc = render_preamble(c, p, out, false);
	if (rc) return rc;
	rc = validate_depth(c, p, d);
	if (rc) return rc;
	for (uint32_t i = 0; i < n; i++)
		if (xy[2u * i] >= p->view.width || xy[2u * i + 1u] >= p->view.height) return fail(c, VR_ERR_INVALID, "pick: a pixel lies outside the window");
	// one launch per query with a one-pixel crop into element i of the context's three arrays, the finishing kernel over all of them, one copy back
	constexpr size_t kXy = 0, kDepth = kXy + VR_PICK_MAX * 2 * sizeof(uint32_t), kValue = kDepth + VR_PICK_MAX * sizeof(float),
	                 kAlpha = kValue + VR_PICK_MAX * sizeof(float), kOut = kAlpha + VR_PICK_MAX * sizeof(float), kBytes = kOut + VR_PICK_MAX * sizeof(vr_pick);
	if (const int grow = grow_buffer(c, &c->pick_stage, c->pick_stage_bytes, kBytes)) return grow;
	uint8_t *stage = (uint8_t *) c->pick_stage;
	VR_TRY(c, hipMemcpyAsync(stage + kXy, xy, (size_t) n * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	vr_params q = *p;
	q.out_width = 1; q.out_rows = 1; q.band_rows = 1; q.band_stride = p->view.height;       // row band_first of bands of one row: frame_row(0) = y
	for (uint32_t i = 0; i < n; i++) {
		q.x0 = xy[2u * i]; q.band_first = xy[2u * i + 1u];
		const vr_depth_out dev = { stage + kDepth + i * sizeof(float), stage + kValue + i * sizeof(float), stage + kAlpha + i * sizeof(float) };
		rc = launch_depth_frame(c, &q, d, &dev, c->stream);
		if (rc) return rc;
	}
	RayKernelArgs a;
	volume_args(c, p, a);
	VR_TRY(c, launch_pick_finish(a, n, (const uint32_t *) (stage + kXy), (const float *) (stage + kDepth), (const float *) (stage + kValue),
	                             (const float *) (stage + kAlpha), (vr_pick *) (stage + kOut), c->stream));
	VR_TRY(c, hipMemcpyAsync(out, stage + kOut, (size_t) n * sizeof(vr_pick), hipMemcpyDeviceToHost, c->stream));
	VR_TRY(c, hipStreamSynchronize(c->stream));
	return VR_OK;
}

int vr_hip_depth_frames(vr_ctx *c, uint64_t *frames_out) { return frames_counted(c, &vr_ctx::depth_frames, frames_out); }

// ---- label volumes (include/vr_hip.h vr_label_entry) ----

namespace {
int set_labels_from(vr_ctx *c, const void *src, bool host, uint32_t x, uint32_t y, uint32_t z) {
	if (c == nullptr) return VR_ERR_INVALID;
	VR_TRY(c, hipSetDevice(c->device));
	if (src == nullptr) {                          // drop
		VR_TRY(c, drain(c));
		drop_labels(c);
		return VR_OK;
	}
	if (c->dim[0] == 0) return fail(c, VR_ERR_NOT_READY, "no volume is resident: labels carry the dims of the volume they belong to (vr_hip_set_volume)");
	if (x != c->dim[0] || y != c->dim[1] || z != c->dim[2]) return fail(c, VR_ERR_INVALID, "label dims differ from the dims of the resident volume");
	VR_TRY(c, drain(c));                         // frames still reading the labels we are about to replace
	const uint64_t elems = (uint64_t) x * y * z, slack = volume_tail_slack(x, y);
	if (c->label_bricks) { (void) hipFree(c->label_bricks); c->label_bricks = nullptr; }
	c->label_bricks_failed = false;
	if (c->labels == nullptr) {
		VR_TRY(c, hipMalloc((void **) &c->labels, elems + slack));
		VR_TRY(c, hipMemsetAsync(c->labels + elems, 0, slack, c->stream));
	}
	const hipError_t e = hipMemcpyAsync(c->labels, src, elems, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream);
	const hipError_t w = hipStreamSynchronize(c->stream);
	if (e != hipSuccess || w != hipSuccess) {
		(void) hipGetLastError();
		drop_labels(c);
		return fail(c, VR_ERR_HIP, "copying the labels failed", e != hipSuccess ? e : w);
	}
	return VR_OK;
}
}  // namespace

int vr_hip_set_labels(vr_ctx *c, const uint8_t *host_labels, uint32_t x, uint32_t y, uint32_t z) { return set_labels_from(c, host_labels, true, x, y, z); }

int vr_hip_set_labels_device(vr_ctx *c, const void *dev_labels, uint32_t x, uint32_t y, uint32_t z) { return set_labels_from(c, dev_labels, false, x, y, z); }

int vr_hip_set_label_table(vr_ctx *c, const vr_label_entry *entries, uint32_t count) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (count > VR_LABEL_COUNT) return fail(c, VR_ERR_INVALID, "a label table has at most 256 entries");
	if (entries == nullptr && count != 0u) return fail(c, VR_ERR_INVALID, "label entries is NULL");
	std::vector<float> table(5u * VR_LABEL_COUNT, 0.0f);
	for (uint32_t i = 0; i < VR_LABEL_COUNT; i++) table[5u * i + 4u] = 1.0f;
	for (uint32_t i = 0; i < count; i++) {
		const float m[5] = { entries[i].colour[0], entries[i].colour[1], entries[i].colour[2], entries[i].mix, entries[i].opacity };
		for (int k = 0; k < 5; k++) {
			if (!std::isfinite(m[k]) || m[k] < 0.0f || m[k] > 1.0f) return fail(c, VR_ERR_INVALID, "label table members must be finite and in [0, 1]");
			table[5u * i + (uint32_t) k] = m[k];
		}
	}
	VR_TRY(c, hipSetDevice(c->device));
	if (const int rc = ensure_label_table(c)) return rc;
	VR_TRY(c, drain(c));                         // frames still reading the table we are about to rewrite
	VR_TRY(c, hipMemcpy(c->label_table, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
	return VR_OK;
}

int vr_hip_render_labelled_device(vr_ctx *c, const vr_params *p, void *dev_rgba, void *stream) {
	return render_to_device(c, p, dev_rgba, stream, [&] { return validate_labelled(c, p); }, [&](hipStream_t on) { return launch_labelled_frame(c, p, dev_rgba, on); });
}

int vr_hip_render_labelled(vr_ctx *c, const vr_params *p, uint8_t *host_rgba) {
	return render_to_host(c, p, host_rgba, nullptr, nullptr, [&] { return validate_labelled(c, p); }, [&](void *) { return launch_labelled_frame(c, p, c->fb, c->stream); });
}

int vr_hip_labelled_frames(vr_ctx *c, uint64_t *frames_out) { return frames_counted(c, &vr_ctx::labelled_frames, frames_out); }

// ---- 2D transfer-function frames (include/vr_hip.h vr_hip_set_tf2d) ----

int vr_hip_set_tf2d(vr_ctx *c, const float *table, uint32_t rows, float g_scale, const uint32_t *esl_bits) {
	if (c == nullptr) return VR_ERR_INVALID;
	VR_TRY(c, hipSetDevice(c->device));
	if (table == nullptr) {
		VR_TRY(c, drain(c));                     // frames still reading the table we are about to drop
		if (c->tf2d_table) { (void) hipFree(c->tf2d_table); c->tf2d_table = nullptr; }
		if (c->tf2d_esl) { (void) hipFree(c->tf2d_esl); c->tf2d_esl = nullptr; }
		c->tf2d_rows = 0;
		return VR_OK;
	}
	if (rows < 2u || rows > VR_TF2D_ROWS_MAX) return fail(c, VR_ERR_INVALID, "a 2-D transfer function has 2..8 rows");
	if (!std::isfinite(g_scale) || g_scale < 0.0f) return fail(c, VR_ERR_INVALID, "g_scale must be finite and not negative");
	if (esl_bits == nullptr) return fail(c, VR_ERR_INVALID, "esl_bits is NULL");
	const size_t members = (size_t) rows * VR_TF_SIZE * 4u;
	for (size_t i = 0; i < members; i++)
		if (!std::isfinite(table[i]) || table[i] < 0.0f) return fail(c, VR_ERR_INVALID, "2-D transfer function members must be finite and not negative");
	// the envelope's leading all-zero entries: every row is zero there (no member is negative, so the maximum is 0 only where all are)
	int zero = -1;
	auto entry_zero = [&](int i) {
		for (uint32_t r = 0; r < rows; r++)
			for (int ch = 0; ch < 4; ch++) if (table[((size_t) r * VR_TF_SIZE + i) * 4u + ch] != 0.0f) return false;
		return true;
	};
	while (zero + 1 < VR_TF_SIZE && entry_zero(zero + 1)) zero++;
	// entry i is g-dependent unless every row holds row 0's bit patterns at i and at min(i + 1, 127)
	uint32_t dependent[4] = { 0, 0, 0, 0 };
	auto same_as_row0 = [&](int i) {
		for (uint32_t r = 1; r < rows; r++)
			if (memcmp(table + ((size_t) r * VR_TF_SIZE + i) * 4u, table + (size_t) i * 4u, 4u * sizeof(float)) != 0) return false;
		return true;
	};
	for (int i = 0; i < VR_TF_SIZE; i++) {
		const int i1 = i + 1 < VR_TF_SIZE ? i + 1 : VR_TF_SIZE - 1;
		if (!same_as_row0(i) || !same_as_row0(i1)) dependent[i >> 5] |= 1u << (i & 31);
	}
	VR_TRY(c, drain(c));                         // frames still reading the table we are about to replace (vr_hip_set_transfer_fn)
	constexpr size_t kTableBytes = (size_t) VR_TF2D_ROWS_MAX * VR_TF_SIZE * 4u * sizeof(float);
	if (c->tf2d_table == nullptr) VR_TRY(c, hipMalloc((void **) &c->tf2d_table, kTableBytes));
	if (c->tf2d_esl == nullptr) VR_TRY(c, hipMalloc((void **) &c->tf2d_esl, VR_ESL_VOLUME_SIZE * sizeof(uint32_t)));
	VR_TRY(c, hipMemsetAsync(c->tf2d_table, 0, kTableBytes, c->stream));
	VR_TRY(c, hipMemcpyAsync(c->tf2d_table, table, members * sizeof(float), hipMemcpyHostToDevice, c->stream));
	VR_TRY(c, hipMemcpyAsync(c->tf2d_esl, esl_bits, VR_ESL_VOLUME_SIZE * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	VR_TRY(c, hipStreamSynchronize(c->stream));
	c->tf2d_rows = rows; c->tf2d_g_scale = g_scale; c->tf2d_zero_below = (float) zero;
	for (int i = 0; i < 4; i++) c->tf2d_g_dependent[i] = dependent[i];
	return VR_OK;
}

int vr_hip_render_tf2d_device(vr_ctx *c, const vr_params *p, void *dev_rgba, void *stream) {
	return render_to_device(c, p, dev_rgba, stream, [&] { return validate_tf2d(c, p); }, [&](hipStream_t on) { return launch_tf2d_frame(c, p, dev_rgba, on); });
}

int vr_hip_render_tf2d(vr_ctx *c, const vr_params *p, uint8_t *host_rgba) {
	return render_to_host(c, p, host_rgba, nullptr, nullptr, [&] { return validate_tf2d(c, p); }, [&](void *) { return launch_tf2d_frame(c, p, c->fb, c->stream); });
}

int vr_hip_tf2d_frames(vr_ctx *c, uint64_t *frames_out) { return frames_counted(c, &vr_ctx::tf2d_frames, frames_out); }

// ---- fused frames (include/vr_hip.h vr_fusion) ----

namespace {
int set_second_from(vr_ctx *c, const void *src, bool host, uint32_t x, uint32_t y, uint32_t z, uint32_t bpv) {
	if (c == nullptr) return VR_ERR_INVALID;
	VR_TRY(c, hipSetDevice(c->device));
	if (src == nullptr) {                          // drop
		VR_TRY(c, drain(c));
		drop_second(c);
		return VR_OK;
	}
	if (c->dim[0] == 0) return fail(c, VR_ERR_NOT_READY, "no volume is resident: a second volume carries the dims and voxel size of the volume it belongs to (vr_hip_set_volume)");
	if (x != c->dim[0] || y != c->dim[1] || z != c->dim[2]) return fail(c, VR_ERR_INVALID, "the second volume's dims differ from the dims of the resident volume");
	if (bpv != c->bpv) return fail(c, VR_ERR_INVALID, "the second volume's bytes_per_voxel differ from the resident volume's");
	VR_TRY(c, drain(c));                         // frames still reading the field we are about to replace
	const uint64_t elems = (uint64_t) x * y * z, slack = volume_tail_slack(x, y);
	void *linear = c->second;                    // (same dims and voxel size: the allocation is reused, the copies are not)
	c->second = nullptr;
	drop_second(c);
	c->second = linear;
	hipError_t e = hipSuccess;
	if (c->second == nullptr) {
		if (hipMalloc(&c->second, (elems + slack) * bpv) != hipSuccess) { (void) hipGetLastError(); c->second = nullptr; return fail(c, VR_ERR_ALLOC, "second volume allocation failed"); }
		e = hipMemsetAsync((uint8_t *) c->second + elems * bpv, 0, slack * bpv, c->stream);
	}
	if (e == hipSuccess) e = hipMemcpyAsync(c->second, src, elems * bpv, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream);
	const hipError_t w = hipStreamSynchronize(c->stream);
	if (e != hipSuccess || w != hipSuccess) {
		(void) hipGetLastError();
		drop_second(c);
		return fail(c, VR_ERR_HIP, "copying the second volume failed", e != hipSuccess ? e : w);
	}
	return VR_OK;
}
}  // namespace

int vr_hip_set_second_volume(vr_ctx *c, const void *host_voxels, uint32_t x, uint32_t y, uint32_t z, uint32_t bpv) { return set_second_from(c, host_voxels, true, x, y, z, bpv); }

int vr_hip_set_second_volume_device(vr_ctx *c, const void *dev_voxels, uint32_t x, uint32_t y, uint32_t z, uint32_t bpv) { return set_second_from(c, dev_voxels, false, x, y, z, bpv); }

int vr_hip_set_second_transfer_fn(vr_ctx *c, const float *tf, const uint32_t *fused_esl_bits) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (tf == nullptr) return fail(c, VR_ERR_INVALID, "the second transfer function is NULL");
	if (fused_esl_bits == nullptr) return fail(c, VR_ERR_INVALID, "fused_esl_bits is NULL: a fused frame leaps by bits of its own (the AND of both fields' bits)");
	for (uint32_t i = 0; i < VR_TF_SIZE * 4u; i++)
		if (!std::isfinite(tf[i]) || tf[i] < 0.0f) return fail(c, VR_ERR_INVALID, "members of the second transfer function must be finite and not negative");
	VR_TRY(c, hipSetDevice(c->device));
	VR_TRY(c, drain(c));                         // frames still reading the function and the bits we are about to replace
	if (c->second_tf == nullptr) VR_TRY(c, hipMalloc((void **) &c->second_tf, VR_TF_SIZE * 4 * sizeof(float)));
	if (c->fused_esl == nullptr) VR_TRY(c, hipMalloc((void **) &c->fused_esl, VR_ESL_VOLUME_SIZE * sizeof(uint32_t)));
	VR_TRY(c, hipMemcpyAsync(c->second_tf, tf, VR_TF_SIZE * 4 * sizeof(float), hipMemcpyHostToDevice, c->stream));
	VR_TRY(c, hipMemcpyAsync(c->fused_esl, fused_esl_bits, VR_ESL_VOLUME_SIZE * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	VR_TRY(c, hipStreamSynchronize(c->stream));
	int zero = -1;                               // the leading all-zero entries, as vr_hip_set_transfer_fn counts them
	while (zero + 1 < VR_TF_SIZE && tf[4 * (zero + 1)] == 0.0f && tf[4 * (zero + 1) + 1] == 0.0f && tf[4 * (zero + 1) + 2] == 0.0f &&
	       tf[4 * (zero + 1) + 3] == 0.0f)
		zero++;
	c->second_zero_below = (float) zero;
	return VR_OK;
}

int vr_hip_render_fused_device(vr_ctx *c, const vr_params *p, const vr_fusion *fusion, void *dev_rgba, void *stream) {
	return render_to_device(c, p, dev_rgba, stream, [&] { return validate_fused(c, p, fusion); }, [&](hipStream_t on) { return launch_fused_frame(c, p, fusion, dev_rgba, on); });
}

int vr_hip_render_fused(vr_ctx *c, const vr_params *p, const vr_fusion *fusion, uint8_t *host_rgba) {
	return render_to_host(c, p, host_rgba, nullptr, nullptr, [&] { return validate_fused(c, p, fusion); }, [&](void *) { return launch_fused_frame(c, p, fusion, c->fb, c->stream); });
}

int vr_hip_fused_frames(vr_ctx *c, uint64_t *frames_out) { return frames_counted(c, &vr_ctx::fused_frames, frames_out); }

#ifdef VR_MIP_STATS
// probe build only (scripts/mip_probe.py): { samples, fetches issued } of the MIP frames that skipped since the last call
int vr_hip_debug_mip_stats(vr_ctx *c, uint64_t *out2) {
	if (c == nullptr || out2 == nullptr) return VR_ERR_INVALID;
	out2[0] = out2[1] = 0;
	if (!c->mip_bounds_ready) return VR_OK;
	VR_TRY(c, hipSetDevice(c->device));
	VR_TRY(c, drain(c));
	VR_TRY(c, hipMemcpy(out2, c->mip_bounds + kMipStatsAt, 16, hipMemcpyDeviceToHost));
	VR_TRY(c, hipMemset(c->mip_bounds + kMipStatsAt, 0, 16));
	return VR_OK;
}
#endif

int vr_hip_timing(vr_ctx *c, vr_timing *out) {
	if (c == nullptr || out == nullptr) return VR_ERR_INVALID;
	(void) hipSetDevice(c->device);
	for (int i = 0; i < kEventRing; i++)
		harvest(c, c->ring[(c->ring_head + i) % kEventRing]);    // oldest first
	out->kernel_ms = c->last_kernel_ms;
	out->total_ms = c->last_total_ms > 0 ? c->last_total_ms : c->last_kernel_ms;
	out->launches = c->launches;
	out->kernel_ms_sum = c->kernel_ms_sum;
	out->kernel_ms_max = c->kernel_ms_max;
	out->total_ms_max = c->total_ms_max;
	return VR_OK;
}

int vr_hip_timing_reset(vr_ctx *c) {
	if (c == nullptr) return VR_ERR_INVALID;
	vr_timing t;
	(void) vr_hip_timing(c, &t);
	c->launches = 0; c->kernel_ms_sum = 0; c->last_kernel_ms = 0; c->last_total_ms = 0; c->kernel_ms_max = 0; c->total_ms_max = 0;
	return VR_OK;
}

int vr_hip_volume_minmax(vr_ctx *c, uint8_t *minmax_out, uint32_t *bd_out, float *bs_out, float *kernel_ms_out) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (minmax_out == nullptr) return fail(c, VR_ERR_INVALID, "minmax_out is NULL");
	if (const int rc = need_linear(c, "set the volume again")) return rc;
	if (c->vol == nullptr) return fail(c, VR_ERR_NOT_READY, "minmax before set_volume");
	VR_TRY(c, hipSetDevice(c->device));
	const uint32_t bd = volume_block_dims(c);
	VR_TRY(c, hipEventRecord(c->aux_start, c->stream));
	VR_TRY(c, launch_minmax(c->vol, c->bpv, c->dim[0], c->dim[1], c->dim[2], bd, c->minmax, c->stream));
	VR_TRY(c, hipEventRecord(c->aux_stop, c->stream));
	VR_TRY(c, hipMemcpyAsync(minmax_out, c->minmax, 32 * 32 * 32 * 2, hipMemcpyDeviceToHost, c->stream));
	VR_TRY(c, hipStreamSynchronize(c->stream));
	if (kernel_ms_out) VR_TRY(c, hipEventElapsedTime(kernel_ms_out, c->aux_start, c->aux_stop));
	if (bd_out) *bd_out = bd;
	if (bs_out) {                                // RaycasterBase.cpp:118-122
		bs_out[0] = 2.0f * (float) bd / (float) c->dim[0];
		bs_out[1] = 2.0f * (float) bd / (float) c->dim[1];
		bs_out[2] = 2.0f * (float) bd / (float) c->dim[2];
	}
	return VR_OK;
}

int vr_hip_volume_histogram(vr_ctx *c, uint64_t *hist_out, float *kernel_ms_out) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (hist_out == nullptr) return fail(c, VR_ERR_INVALID, "hist_out is NULL");
	if (const int rc = need_linear(c, "set the volume again")) return rc;
	if (c->vol == nullptr) return fail(c, VR_ERR_NOT_READY, "histogram before set_volume");
	VR_TRY(c, hipSetDevice(c->device));
	VR_TRY(c, hipEventRecord(c->aux_start, c->stream));
	VR_TRY(c, launch_histogram(c->vol, c->bpv, c->vol_elems, c->hist, c->stream));
	VR_TRY(c, hipEventRecord(c->aux_stop, c->stream));
	VR_TRY(c, hipMemcpyAsync(hist_out, c->hist, 256 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
	VR_TRY(c, hipStreamSynchronize(c->stream));
	if (kernel_ms_out) VR_TRY(c, hipEventElapsedTime(kernel_ms_out, c->aux_start, c->aux_stop));
	return VR_OK;
}

int vr_hip_gradient_histogram(vr_ctx *c, uint32_t g_bins, float g_scale, uint64_t *hist_out, float *kernel_ms_out) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (hist_out == nullptr) return fail(c, VR_ERR_INVALID, "hist_out is NULL");
	if (g_bins < 1u || g_bins > VR_GRADIENT_BINS_MAX) return fail(c, VR_ERR_INVALID, "g_bins must be in 1..32");
	if (!std::isfinite(g_scale) || g_scale < 0.0f) return fail(c, VR_ERR_INVALID, "g_scale must be finite and not negative");
	if (const int rc = need_linear(c, "set the volume again")) return rc;
	if (c->vol == nullptr) return fail(c, VR_ERR_NOT_READY, "histogram before set_volume");
	VR_TRY(c, hipSetDevice(c->device));
	if (c->gradient_hist == nullptr) VR_TRY(c, hipMalloc((void **) &c->gradient_hist, (size_t) VR_GRADIENT_BINS_MAX * 256u * sizeof(unsigned long long)));
	const RayKernelArgs *bc = nullptr;
#ifdef VR_BOUNDS_CHECK
	// the net of the debug build: every load of the kernel is held against the linear array (without its tail slack: no voxel lies there)
	vr_params none;
	memset(&none, 0, sizeof none);
	RayKernelArgs a;
	volume_args(c, &none, a);
	if (c->bc_fault == nullptr) {
		VR_TRY(c, hipMalloc((void **) &c->bc_fault, 8 * sizeof(uint32_t)));
		VR_TRY(c, hipMemset(c->bc_fault, 0, 8 * sizeof(uint32_t)));
	}
	a.bc_base = (uint64_t) (uintptr_t) c->vol; a.bc_bytes = c->vol_elems * c->bpv; a.bc_fault = c->bc_fault;
	bc = &a;
#endif
	VR_TRY(c, hipEventRecord(c->aux_start, c->stream));
	VR_TRY(c, launch_gradient_histogram(c->vol, c->bpv, c->dim, g_bins, g_scale, c->gradient_hist, bc, c->stream));
	VR_TRY(c, hipEventRecord(c->aux_stop, c->stream));
	VR_TRY(c, hipMemcpyAsync(hist_out, c->gradient_hist, (size_t) g_bins * 256u * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
	VR_TRY(c, hipStreamSynchronize(c->stream));
#ifdef VR_BOUNDS_CHECK
	{ const int verdict = bounds_check_verdict(c, c->stream, kLayoutLinear); if (verdict) return verdict; }
#endif
	if (kernel_ms_out) VR_TRY(c, hipEventElapsedTime(kernel_ms_out, c->aux_start, c->aux_stop));
	return VR_OK;
}

int vr_hip_generate_volume(vr_ctx *c, uint32_t kind, uint32_t n, uint32_t seed, uint32_t bpv) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (kind > 1) return fail(c, VR_ERR_INVALID, "unknown synthetic volume kind");
	VR_TRY(c, hipSetDevice(c->device));
	int rc = alloc_volume(c, n, n, n, bpv);
	if (rc) return rc;
	const auto t0 = std::chrono::steady_clock::now();
	VR_TRY(c, launch_generate(c->vol, kind, n, seed, bpv, c->stream));
	VR_TRY(c, hipStreamSynchronize(c->stream));
	c->upload_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
	return VR_OK;
}

int vr_hip_download_volume(vr_ctx *c, void *host_out, uint64_t bytes) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (host_out == nullptr) return fail(c, VR_ERR_INVALID, "host_out is NULL");
	if (const int rc = need_linear(c, "set the volume again")) return rc;
	if (c->vol == nullptr) return fail(c, VR_ERR_NOT_READY, "download before set_volume");
	if (bytes != c->vol_elems * c->bpv) return fail(c, VR_ERR_INVALID, "byte count does not match the resident volume");
	VR_TRY(c, hipSetDevice(c->device));
	VR_TRY(c, hipMemcpy(host_out, c->vol, bytes, hipMemcpyDeviceToHost));
	return VR_OK;
}

int vr_hip_volume_info(vr_ctx *c, vr_volume_info *out) {
	if (c == nullptr || out == nullptr) return VR_ERR_INVALID;
	memset(out, 0, sizeof *out);
	if (c->dim[0] == 0) return fail(c, VR_ERR_NOT_READY, "volume_info before set_volume");
	out->dim_x = c->dim[0]; out->dim_y = c->dim[1]; out->dim_z = c->dim[2]; out->bytes_per_voxel = c->bpv;
	out->layout = c->layout;
	out->linear_resident = c->vol != nullptr ? 1u : 0u;
	out->linear_bytes = c->vol != nullptr ? (c->vol_elems + volume_tail_slack(c->dim[0], c->dim[1])) * c->bpv : 0;
	for (uint32_t k = 0; k < kCopyKinds; k++) {
		out->build_ms[k] = c->copy_build_ms[k];
		if (copy_in_policy(c, k)) out->copies_in_policy |= 1u << k;
		if (c->copy_failed[k]) out->copies_refused |= 1u << k;
		if (c->copy[k] == nullptr) continue;
		out->copies |= 1u << k;
		out->bricked_bytes += copy_bytes(c, k);
		if (k <= kCopyQuadYZ) { out->brick_planes |= 1u << k; out->brick_copies++; }
	}
	// the aligned run bricks: their own bits and their bytes (build times: vr_hip_run_aligned_info — this struct's size is pinned)
	for (uint32_t k = kCopyRun7Z; k <= kCopyRun7Y; k++) {
		if (c->copy[k]) { out->copies |= 1u << k; out->bricked_bytes += copy_bytes(c, k); }
		if (c->copy_failed[k]) out->copies_refused |= 1u << k;
	}
	if (c->copy[kCopyRunZ]) out->run_copy |= 1u;
	if (c->copy[kCopyRunY]) out->run_copy |= 2u;
	if (c->copy[kCopyVoxel]) out->run_copy |= 4u;
	out->brick_copies_wanted = (c->layout == VR_LAYOUT_BRICKED) ? (copy_in_policy(c, kCopyQuadXZ) ? 3u : 1u) : 0u;
	out->upload_ms = c->upload_ms;
	return VR_OK;
}

int vr_hip_prepare(vr_ctx *c, uint32_t copies) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (c->dim[0] == 0) return fail(c, VR_ERR_NOT_READY, "prepare before set_volume");
	if (copies & ~((1u << kCopySlots) - 1u)) return fail(c, VR_ERR_INVALID, "unknown copy bits");
	VR_TRY(c, hipSetDevice(c->device));
	int worst = VR_OK;
	for (uint32_t k = 0; k < kCopySlots; k++) {
		if (!((copies >> k) & 1u) || c->copy[k] || !copy_in_policy(c, k)) continue;      // copies the policy does not have at this size are skipped
		if (const int rc = need_linear(c, "set the volume again")) return rc;
		c->copy_failed[k] = false;                   // an explicit request retries an earlier refusal
		const int rc = build_copy(c, k);
		if (rc != VR_OK && worst == VR_OK) { worst = rc; if (c->err.empty() || rc == VR_ERR_ALLOC) fail(c, rc, "a brick copy was not built (less than half of the HBM would stay free, or allocation failed)"); }
	}
	if (copies) forget_tile_mappings(c);
	return worst;
}

int vr_hip_download_copy(vr_ctx *c, uint32_t kind, void *host_out, uint64_t capacity, uint64_t *bytes_out) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (kind >= kCopySlots) return fail(c, VR_ERR_INVALID, "unknown copy kind");
	if (c->copy[kind] == nullptr) return fail(c, VR_ERR_NOT_READY, "this brick copy is not resident (render a frame that reads it, or vr_hip_prepare)");
	uint64_t bytes = copy_bytes(c, kind);
	if (kind == kCopyRunZ || kind == kCopyRunY || kind == kCopyRun7Z || kind == kCopyRun7Y) bytes -= 16;     // the allocation's tail slack is not part of the copy
	if (bytes_out) *bytes_out = bytes;
	if (host_out == nullptr) return VR_OK;
	if (capacity < bytes) return fail(c, VR_ERR_INVALID, "buffer too small for this copy");
	VR_TRY(c, hipSetDevice(c->device));
	VR_TRY(c, drain(c));
	VR_TRY(c, hipMemcpy(host_out, c->copy[kind], bytes, hipMemcpyDeviceToHost));
	return VR_OK;
}

int vr_hip_release_linear_copy(vr_ctx *c) {
	if (c == nullptr) return VR_ERR_INVALID;
	if (c->dim[0] == 0) return fail(c, VR_ERR_NOT_READY, "release_linear_copy before set_volume");
	if (c->vol == nullptr) return VR_OK;
	bool any = false;
	for (uint32_t k = 0; k < kCopySlots; k++) any = any || c->copy[k] != nullptr;
	if (!any || max_dim_of(c) > 2048u)
		return fail(c, VR_ERR_INVALID, "the linear array is the only copy a render path can read (no brick copy resident: render a frame or call "
		                               "vr_hip_prepare first; linear layout; or an edge above 2048)");
	if (c->force_wide == 1u)
		return fail(c, VR_ERR_INVALID, "the index-arithmetic path (vr_hip_set_wide_addressing 1) reads the linear array");
	VR_TRY(c, hipSetDevice(c->device));
	VR_TRY(c, drain(c));
	const int rc = build_mip_bounds(c);          // MIP frames with esl on need the scan of the linear array: taken now (64 KiB)
	if (rc) return rc;
	(void) hipFree(c->vol);
	c->vol = nullptr;
	return VR_OK;
}

int vr_hip_device_info(vr_ctx *c, char *name_out, size_t name_cap, uint32_t *cus, uint64_t *hbm_bytes) {
	if (c == nullptr) return VR_ERR_INVALID;
	hipDeviceProp_t prop;
	VR_TRY(c, hipGetDeviceProperties(&prop, c->device));
	if (name_out && name_cap) { snprintf(name_out, name_cap, "%s (%s)", prop.name, prop.gcnArchName); }
	if (cus) *cus = (uint32_t) prop.multiProcessorCount;
	if (hbm_bytes) *hbm_bytes = (uint64_t) prop.totalGlobalMem;
	return VR_OK;
}

}  // extern "C"
