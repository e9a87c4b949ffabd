// HipRenderer.cpp — the Renderer back-end that forwards the reference's five virtuals to the C ABI (include/vr_hip.h).
// Return conventions follow the reference: 0 = ok, 1 = failure (CPURenderer.cpp:44-45, GPURenderer1.cu:91-95,101-102);
// nothing here exits the process (the reference's cuda_safe_call does, cuda_utils.h:25-31 — deliberately not mirrored).
#include "Renderer.h"

namespace volr {

static void copy3(float *dst, const float3 &v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; }

void HipRenderer::to_params(const Raycaster &r, vr_sampling sampling, vr_params *p) {
	p->view.width = r.view.dims.x;
	p->view.height = r.view.dims.y;
	copy3(p->view.origin, r.view.origin);
	copy3(p->view.direction, r.view.direction);
	copy3(p->view.right_plane, r.view.right_plane);
	copy3(p->view.up_plane, r.view.up_plane);
	copy3(p->view.light_pos, r.view.light_pos);
	p->view.perspective = r.view.perspective ? 1u : 0u;
	p->ray_step = r.ray_step;
	p->ray_threshold = r.ray_threshold;
	p->esl = r.esl ? 1u : 0u;
	p->esl_block_dims = r.esl_block_dims;
	copy3(p->esl_block_size, r.esl_block_size);
	p->light_kd = r.light_kd;
	p->sampling = (uint32_t) sampling;
	p->x0 = 0;
	p->out_width = r.view.dims.x;
	p->out_rows = r.view.dims.y;
	p->band_rows = r.view.dims.y ? r.view.dims.y : 1;
	p->band_stride = 1;
	p->band_first = 0;
}

// The refusal of a device list, stated once; string literals, because mirror_error_ is a const char *.
#define SINGLE_DEVICE(what, entry) what " a single device (" entry "): construct the renderer without a device list"

// per Kind, in the enum's order: what render_volume() says to a device list (the composite is the one kind that renders on one)
static const char *const kind_single_device[] = {
	nullptr,
	SINGLE_DEVICE("the maximum-intensity projection renders on", "vr_hip_render_mip"),
	SINGLE_DEVICE("the isosurface renders on", "vr_hip_render_iso"),
	SINGLE_DEVICE("the hybrid renders on", "vr_hip_render_hybrid"),
	SINGLE_DEVICE("a section frame renders on", "vr_hip_render_section"),
	SINGLE_DEVICE("a section frame renders on", "vr_hip_render_section"),
	SINGLE_DEVICE("a labelled frame renders on", "vr_hip_render_labelled"),
};

static int status(int rc) { return rc == 0 ? 0 : 1; }

HipRenderer::HipRenderer(Raycaster r, int device, vr_sampling sampling, bool device_buffer) : sampling_(sampling), device_buffer_(device_buffer) {
	create_status_ = vr_hip_create(device, &ctx_);
	if (create_status_ == 0)
		prime(r);
}

HipRenderer::HipRenderer(Raycaster r, const int *devices, int n_devices, vr_sampling sampling, bool device_buffer) : sampling_(sampling), device_buffer_(device_buffer) {
	create_status_ = vr_hip_multi_create(n_devices, devices, &multi_);
	if (create_status_ == 0)
		prime(r);
}

// GPURenderer1.cu:17-21: the constructor primes window, TF and volume from the Raycaster it is given
void HipRenderer::prime(const Raycaster &r) {
	if (r.view.dims.x != 0 && r.view.dims.y != 0)
		set_window_buffer(r.view);
	if (r.transfer_fn != nullptr && r.esl_volume != nullptr)
		set_transfer_fn(r);
	if (r.volume.data != nullptr)
		set_volume(r.volume);
}

HipRenderer::~HipRenderer() {
	vr_hip_destroy(ctx_);
	vr_hip_multi_destroy(multi_);
}

const char *HipRenderer::last_error() const {
	if (mirror_error_ != nullptr)
		return mirror_error_;
	if (multi_ != nullptr)
		return vr_hip_multi_last_error(multi_);
	if (ctx_ == nullptr)
		return create_status_ == VR_ERR_NO_DEVICE ? "no usable HIP device (there is no CPU fallback)" : "context creation failed";
	return vr_hip_last_error(ctx_);
}

bool HipRenderer::open() {
	if (!ok())
		return false;
	mirror_error_ = nullptr;
	return true;
}

bool HipRenderer::single_device(const char *refusal) {
	if (multi_ == nullptr)
		return true;
	mirror_error_ = refusal;
	return false;
}

template <typename... Params, typename... Args>
int HipRenderer::forward(int (*on_list)(vr_multi *, Params...), int (*on_context)(vr_ctx *, Params...), Args... args) {
	return status(multi_ ? on_list(multi_, args...) : on_context(ctx_, args...));
}

// the three virtuals of the reference keep a standing refusal of this class; the setters of this class alone clear it (open())
void HipRenderer::set_window_buffer(View view) {
	if (ok())
		forward(vr_hip_multi_set_window, vr_hip_set_window, view.dims.x, view.dims.y);
}

void HipRenderer::set_transfer_fn(Raycaster r) {
	if (ok())
		forward(vr_hip_multi_set_transfer_fn, vr_hip_set_transfer_fn, (const float *) r.transfer_fn, r.esl_volume);
}

int HipRenderer::set_volume(Model volume) {
	return ok() ? forward(vr_hip_multi_set_volume, vr_hip_set_volume, volume.data, volume.dims.x, volume.dims.y, volume.dims.z, 1) : 1;
}

int HipRenderer::set_clip(const vr_clip *clip) { return open() ? forward(vr_hip_multi_set_clip, vr_hip_set_clip, clip) : 1; }

int HipRenderer::set_shadow(const vr_shadow *shadow) { return open() ? forward(vr_hip_multi_set_shadow, vr_hip_set_shadow, shadow) : 1; }

int HipRenderer::set_lighting(const vr_lighting *lighting) { return open() ? forward(vr_hip_multi_set_lighting, vr_hip_set_lighting, lighting) : 1; }

int HipRenderer::set_preintegration(bool on) { return open() ? forward(vr_hip_multi_set_preintegration, vr_hip_set_preintegration, on ? 1u : 0u) : 1; }

int HipRenderer::render_volume(uchar4 *buffer, Raycaster r) {
	if (buffer == nullptr || !open())
		return 1;
	if (kind_ != Kind::composite && !single_device(kind_single_device[(int) kind_]))
		return 1;
	vr_params p;
	to_params(r, sampling_, &p);
	uint8_t *const host = (uint8_t *) buffer;
	if (device_buffer_)
		switch (kind_) {
			case Kind::composite: return status(multi_ ? vr_hip_multi_render_device(multi_, &p, buffer) : vr_hip_render_device(ctx_, &p, buffer, nullptr));
			case Kind::mip: return status(vr_hip_render_mip_device(ctx_, &p, buffer, nullptr));
			case Kind::iso: return status(vr_hip_render_iso_device(ctx_, &p, &iso_params_, buffer, nullptr, nullptr));
			case Kind::hybrid: return status(vr_hip_render_hybrid_device(ctx_, &p, &iso_params_, buffer, nullptr, nullptr));
			case Kind::section: return status(vr_hip_render_section_device(ctx_, &p, &section_params_, buffer, nullptr, nullptr));
			case Kind::section_in_volume: return status(vr_hip_render_section_in_volume_device(ctx_, &p, &section_params_, buffer, nullptr, nullptr));
			case Kind::labelled: return status(vr_hip_render_labelled_device(ctx_, &p, buffer, nullptr));
		}
	else
		switch (kind_) {
			case Kind::composite: return status(multi_ ? vr_hip_multi_render(multi_, &p, host) : vr_hip_render(ctx_, &p, host));
			case Kind::mip: return status(vr_hip_render_mip(ctx_, &p, host));
			case Kind::iso: return status(vr_hip_render_iso(ctx_, &p, &iso_params_, host, nullptr));
			case Kind::hybrid: return status(vr_hip_render_hybrid(ctx_, &p, &iso_params_, host, nullptr));
			case Kind::section: return status(vr_hip_render_section(ctx_, &p, &section_params_, host, nullptr));
			case Kind::section_in_volume: return status(vr_hip_render_section_in_volume(ctx_, &p, &section_params_, host, nullptr));
			case Kind::labelled: return status(vr_hip_render_labelled(ctx_, &p, host));
		}
	return 1;
}

int HipRenderer::render_backdrop(uchar4 *buffer, Raycaster r, const vr_backdrop *layer) {
	if (buffer == nullptr || !open() || !single_device(SINGLE_DEVICE("a backdrop frame renders on", "vr_hip_render_backdrop")))
		return 1;
	vr_params p;
	to_params(r, sampling_, &p);
	return status(device_buffer_ ? vr_hip_render_backdrop_device(ctx_, &p, layer, buffer, nullptr) : vr_hip_render_backdrop(ctx_, &p, layer, (uint8_t *) buffer));
}

int HipRenderer::set_labels(const uint8_t *labels, const uint32_t dims[3]) {
	if (!open() || !single_device(SINGLE_DEVICE("label volumes belong to", "vr_hip_set_labels")))
		return 1;
	return status(vr_hip_set_labels(ctx_, labels, dims ? dims[0] : 0u, dims ? dims[1] : 0u, dims ? dims[2] : 0u));
}

int HipRenderer::set_label_table(const vr_label_entry *entries, uint32_t count) {
	if (!open() || !single_device(SINGLE_DEVICE("label tables belong to", "vr_hip_set_label_table")))
		return 1;
	return status(vr_hip_set_label_table(ctx_, entries, count));
}

int HipRenderer::render_depth(Raycaster r, const vr_depth &depth, const vr_depth_out *out) {
	if (out == nullptr || !open() || !single_device(SINGLE_DEVICE("a depth frame renders on", "vr_hip_render_depth")))
		return 1;
	vr_params p;
	to_params(r, sampling_, &p);
	return status(device_buffer_ ? vr_hip_render_depth_device(ctx_, &p, &depth, out, nullptr) : vr_hip_render_depth(ctx_, &p, &depth, out));
}

int HipRenderer::pick(Raycaster r, const vr_depth &depth, uint32_t n, const uint32_t *xy, vr_pick *out) {
	if (!open() || !single_device(SINGLE_DEVICE("a pick renders on", "vr_hip_pick")))
		return 1;
	vr_params p;
	to_params(r, sampling_, &p);
	return status(vr_hip_pick(ctx_, &p, &depth, n, xy, out));
}

}  // namespace volr
