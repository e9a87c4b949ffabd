// Renderer.h — host-side C++ mirror of the reference's renderer plug-in interface, for the ONE back-end this
// project provides: HipRenderer (MI355X).  Same class / method / field names, argument meaning and return
// conventions as the reference (VolumeRendering/Renderer.h:13-28, RaycasterBase.h:20-30, ModelBase.h:11-15,
// ViewBase.h:14-21), so a call site written against the reference compiles against this header unchanged
// (inside namespace volr) and tests read like the reference's own call sequences.
//
// All GPU work happens below the C ABI of include/vr_hip.h; this file contains no HIP calls.
#pragma once

#include <hip/hip_vector_types.h>   // float3 / float4 / uchar4 / ushort2 / ushort3 / short2 PODs (HIP's own, not CUDA's)
#include "../../../include/vr_hip.h"

namespace volr {

typedef unsigned int esl_type;      // RaycasterBase.h:18

constexpr int TF_SIZE = VR_TF_SIZE;
constexpr int TF_RATIO = VR_TF_RATIO;
constexpr int ESL_VOLUME_DIMS = VR_ESL_VOLUME_DIMS;
constexpr int ESL_VOLUME_SIZE = VR_ESL_VOLUME_SIZE;
constexpr int ESL_MIN_BLOCK_SIZE = VR_ESL_MIN_BLOCK;

// ModelBase.h:11-15.  `data` stays owned by the caller; renderers copy it in set_volume().
struct Model {
	unsigned char *data;
	unsigned int size;
	ushort3 dims;
	float3 min_bound;               // always (-1,-1,-1) (ModelBase.cpp:10-14)
};

// ViewBase.h:14-21
struct View {
	ushort2 dims;
	float3 origin;
	float3 direction;
	float3 right_plane;
	float3 up_plane;
	float3 light_pos;
	bool perspective;
};

// RaycasterBase.h:20-30 (the per-ray methods of the reference struct live in the HIP kernel, not here)
struct Raycaster {
	Model volume;
	View view;
	float4 *transfer_fn;            // TF_SIZE premultiplied entries, owned by RaycasterBase
	float ray_step;
	float ray_threshold;
	bool esl;
	esl_type *esl_volume;           // ESL_VOLUME_SIZE words, bit set = block empty, owned by RaycasterBase
	unsigned short esl_block_dims;
	float3 esl_block_size;
	float light_kd;
};

// Renderer.h:13-28
class Renderer {
	public:
		virtual ~Renderer() {}
		virtual const char *get_name() { return "Default"; }
		virtual void set_window_buffer(View) {}
		virtual void set_transfer_fn(Raycaster) {}
		virtual int set_volume(Model) { return 0; }
		virtual int render_volume(uchar4 *buffer, Raycaster r) = 0;
};

// The MI355X back-end.  Construction performs the three set_* calls like every reference GPU renderer
// (GPURenderer1.cu:17-21).  `buffer` of render_volume() is a HOST pointer by default (reference renderer ids 0-2,
// VolR.cpp:76-87) or a DEVICE pointer when constructed with device_buffer = true (ids 3-4).
class HipRenderer : public Renderer {
	public:
		explicit HipRenderer(Raycaster r, int device = 0, vr_sampling sampling = VR_SAMPLE_TRILINEAR, bool device_buffer = false);
		// several GPUs behind the same five virtuals (include/vr_hip.h vr_hip_multi_*): the frame is split into interleaved bands,
		// gathered on devices[0]; with device_buffer the `buffer` of render_volume() is a device pointer on devices[0]
		HipRenderer(Raycaster r, const int *devices, int n_devices, vr_sampling sampling = VR_SAMPLE_TRILINEAR, bool device_buffer = false);
		virtual ~HipRenderer();
		virtual const char *get_name() { return sampling_ == VR_SAMPLE_NEAREST ? "HIP MI355X nearest" : (sampling_ == VR_SAMPLE_TRILINEAR_Q8 ? "HIP MI355X trilinear q8" : "HIP MI355X trilinear"); }
		virtual void set_window_buffer(View view);
		virtual void set_transfer_fn(Raycaster r);
		virtual int set_volume(Model volume);
		virtual int render_volume(uchar4 *buffer, Raycaster r);

		bool ok() const { return (ctx_ != nullptr || multi_ != nullptr) && create_status_ == 0; }
		const char *last_error() const;
		vr_ctx *context() { return multi_ ? vr_hip_multi_context(multi_, 0) : ctx_; }
		vr_multi *multi() { return multi_; }
		void set_sampling(vr_sampling s) { sampling_ = s; }
		// true: render_volume() produces the maximum-intensity projection (vr_hip_render_mip: the largest sample of every ray through one
		// transfer-function lookup; Raycaster::esl then selects its exact fetch skipping) instead of the front-to-back composite.
		// Single device only: with a device list render_volume() returns 1 and last_error() says why.
		void set_mip(bool mip) { hold(Kind::mip, mip); }
		// on: render_volume() produces the shaded isosurface at `level` (raw voxel units) with `refine` bisection steps (vr_hip_render_iso;
		// Raycaster::esl selects its exact fetch skipping, no depth comes back through this interface).  Needs a TRILINEAR sampling mode.
		// Excludes set_mip: the one set last holds.  Single device only, like set_mip.
		void set_iso(bool on, float level, uint32_t refine) { iso_params_ = { level, refine }; hold(Kind::iso, on); }
		// on: render_volume() produces the hybrid (vr_hip_render_hybrid): that isosurface seen through the translucent volume in front of it —
		// the isosurface frame, then the composite frame stopped at its depth and blended over it; the composite pass sees the clip, the
		// shadow, the lighting and the pre-integration of this renderer.  Needs a TRILINEAR sampling mode.  Excludes set_mip and set_iso:
		// the one set last holds.  Single device only, like them.
		void set_hybrid(bool on, float level, uint32_t refine) { iso_params_ = { level, refine }; hold(Kind::hybrid, on); }
		// on: render_volume() produces the section frame (vr_hip_render_section): the oblique slice `section` through the interpolated field, or
		// its thick-slab maximum, minimum or mean, coloured by the transfer function or the section's grey window; in_volume: that section seen
		// through the translucent volume in front of it (vr_hip_render_section_in_volume: the composite pass sees the clip, the shadow, the
		// lighting and the pre-integration of this renderer).  No depth comes back through this interface.  Needs a TRILINEAR sampling mode.
		// Excludes set_mip, set_iso and set_hybrid: the one set last holds.  Single device only, like them.
		void set_section(bool on, const vr_section &section, bool in_volume) {
			section_params_ = section;
			if (kind_ == Kind::section_in_volume) kind_ = Kind::section;      // the two section kinds are one to this setter: off leaves either
			hold(Kind::section, on);
			if (on && in_volume) kind_ = Kind::section_in_volume;
		}
		// One composite frame over an opaque layer (vr_hip_render_backdrop / vr_hip_render_backdrop_device by the buffer flavour of this
		// renderer): `layer` holds host or device pointers accordingly, view.dims pixels each.  Whatever set_mip / set_iso / set_hybrid say,
		// this is a composite frame.  Single device only.  0 = ok, 1 = failure.
		int render_backdrop(uchar4 *buffer, Raycaster r, const vr_backdrop *layer);
		// One depth frame of the composite (vr_hip_render_depth / vr_hip_render_depth_device by the buffer flavour of this renderer): `out`
		// holds host or device pointers accordingly, view.dims floats each; value and alpha may be NULL.  The clip and the pre-integration
		// of this renderer apply.  Needs a TRILINEAR sampling mode.  Single device only.  0 = ok, 1 = failure.
		int render_depth(Raycaster r, const vr_depth &depth, const vr_depth_out *out);
		// What that depth frame stores at each of the n pixels xy[2i], xy[2i + 1] (y up), with the position and the voxel index of a hit
		// (vr_hip_pick: host arrays, synchronous, at most 256 pixels).  Single device only.  0 = ok, 1 = failure.
		int pick(Raycaster r, const vr_depth &depth, uint32_t n, const uint32_t *xy, vr_pick *out);
		// Label volumes (vr_hip_set_labels, vr_hip_set_label_table, vr_hip_render_labelled*): one byte per voxel with the dims of the resident
		// volume (NULL drops them; a new volume drops them too), and what each of the 256 labels does to a sample's classified colour (entries
		// beyond `count`, and all of them for NULL / 0, are the identity).  set_labelled(true): render_volume() produces the labelled composite
		// frame — the clip, the shadow and the lighting of this renderer apply; it needs a TRILINEAR sampling mode and excludes the
		// pre-integration, set_mip, set_iso, set_hybrid and set_section: the one set last holds.  Single device only.  0 = ok, 1 = failure.
		int set_labels(const uint8_t *labels, const uint32_t dims[3]);
		int set_label_table(const vr_label_entry *entries, uint32_t count);
		void set_labelled(bool on) { hold(Kind::labelled, on); }
		// The clip region of every later frame of this renderer — composite, set_mip and set_iso alike, and with a device list every device's
		// bands (vr_hip_set_clip / vr_hip_multi_set_clip: a crop box in model space and a kept half-space).  NULL switches clipping off.
		// 0 = ok, 1 = failure (a non-finite member, box_min >= box_max), the reference's convention.
		int set_clip(const vr_clip *clip);
		// Light-source shadows of every later COMPOSITE frame of this renderer (vr_hip_set_shadow / vr_hip_multi_set_shadow: a light grid
		// marched towards shadow->light_pos, one more filtered fetch per dense sample); set_mip and set_iso frames ignore it.  NULL = off.
		int set_shadow(const vr_shadow *shadow);
		// Gradient lighting of every later COMPOSITE frame of this renderer (vr_hip_set_lighting / vr_hip_multi_set_lighting: Blinn-Phong from
		// the gradient of the interpolated field in place of the reference's cue; light_kd is then ignored); set_mip and set_iso frames
		// ignore it.  clear_lighting() = set_lighting(NULL) = off.  0 = ok, 1 = failure (a coefficient outside 0..1, shininess_log2 > 10).
		int set_lighting(const vr_lighting *lighting);
		int clear_lighting() { return set_lighting(nullptr); }
		// Pre-integrated (slab) classification of every later COMPOSITE frame of this renderer (vr_hip_set_preintegration /
		// vr_hip_multi_set_preintegration: a sample takes the mean of the transfer function between the previous sample's value and its own);
		// set_mip and set_iso frames ignore it; clip, shadow and lighting compose with it.  false = off, the default.  0 = ok, 1 = failure.
		int set_preintegration(bool on);
		// fills the by-value parameter block from a Raycaster (whole-frame partition)
		static void to_params(const Raycaster &r, vr_sampling sampling, vr_params *out);
	private:
		HipRenderer(const HipRenderer &);
		HipRenderer &operator=(const HipRenderer &);
		// what render_volume() produces: one kind at a time, so a setter that switches its kind on replaces whichever held before
		enum class Kind { composite, mip, iso, hybrid, section, section_in_volume, labelled };
		void hold(Kind kind, bool on) { if (on) kind_ = kind; else if (kind_ == kind) kind_ = Kind::composite; }
		void prime(const Raycaster &r);
		bool open();                                    // ok(), and then no failure of this class stands any more
		bool single_device(const char *refusal);       // false with `refusal` as last_error() when there is a device list
		// one setter on the device list or on the context; 0 = ok, 1 = failure
		template <typename... Params, typename... Args>
		int forward(int (*on_list)(vr_multi *, Params...), int (*on_context)(vr_ctx *, Params...), Args... args);
		vr_ctx *ctx_ = nullptr;
		vr_multi *multi_ = nullptr;
		int create_status_ = 0;
		vr_sampling sampling_;
		bool device_buffer_;
		Kind kind_ = Kind::composite;
		vr_iso iso_params_ = { 0.0f, 0u };             // of Kind::iso and Kind::hybrid: stored by their setters whether or not `on`
		vr_section section_params_ = {};               // of the two section kinds, likewise
		const char *mirror_error_ = nullptr;            // a failure of this class itself (nothing below the C ABI was called)
};

}  // namespace volr
