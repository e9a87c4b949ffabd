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

HipRenderer::HipRenderer(Raycaster r, int device, vr_sampling sampling, bool device_buffer)
	: ctx_(nullptr), multi_(nullptr), create_status_(0), sampling_(sampling), device_buffer_(device_buffer), mip_(false), iso_(false), hybrid_(false), iso_params_{ 0.0f, 0u }, section_(false), section_in_volume_(false), section_params_{}, labelled_(false), mirror_error_(nullptr) {
	create_status_ = vr_hip_create(device, &ctx_);
	if (create_status_ == 0)
		prime(r);
}

HipRenderer::HipRenderer(Raycaster r, const int *devices, int n_devices, vr_sampling sampling, bool device_buffer)
	: ctx_(nullptr), multi_(nullptr), create_status_(0), sampling_(sampling), device_buffer_(device_buffer), mip_(false), iso_(false), hybrid_(false), iso_params_{ 0.0f, 0u }, section_(false), section_in_volume_(false), section_params_{}, labelled_(false), mirror_error_(nullptr) {
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

void HipRenderer::set_window_buffer(View view) {
	if (!ok())
		return;
	if (multi_) vr_hip_multi_set_window(multi_, view.dims.x, view.dims.y);
	else vr_hip_set_window(ctx_, view.dims.x, view.dims.y);
}

void HipRenderer::set_transfer_fn(Raycaster r) {
	if (!ok())
		return;
	if (multi_) vr_hip_multi_set_transfer_fn(multi_, (const float *) r.transfer_fn, r.esl_volume);
	else vr_hip_set_transfer_fn(ctx_, (const float *) r.transfer_fn, r.esl_volume);
}

int HipRenderer::set_volume(Model volume) {
	if (!ok())
		return 1;
	int rc = multi_ ? vr_hip_multi_set_volume(multi_, volume.data, volume.dims.x, volume.dims.y, volume.dims.z, 1)
	                : vr_hip_set_volume(ctx_, volume.data, volume.dims.x, volume.dims.y, volume.dims.z, 1);
	return rc == 0 ? 0 : 1;
}

int HipRenderer::set_clip(const vr_clip *clip) {
	if (!ok())
		return 1;
	mirror_error_ = nullptr;
	const int rc = multi_ ? vr_hip_multi_set_clip(multi_, clip) : vr_hip_set_clip(ctx_, clip);
	return rc == 0 ? 0 : 1;
}

int HipRenderer::set_shadow(const vr_shadow *shadow) {
	if (!ok())
		return 1;
	mirror_error_ = nullptr;
	const int rc = multi_ ? vr_hip_multi_set_shadow(multi_, shadow) : vr_hip_set_shadow(ctx_, shadow);
	return rc == 0 ? 0 : 1;
}

int HipRenderer::set_lighting(const vr_lighting *lighting) {
	if (!ok())
		return 1;
	mirror_error_ = nullptr;
	const int rc = multi_ ? vr_hip_multi_set_lighting(multi_, lighting) : vr_hip_set_lighting(ctx_, lighting);
	return rc == 0 ? 0 : 1;
}

int HipRenderer::set_preintegration(bool on) {
	if (!ok())
		return 1;
	mirror_error_ = nullptr;
	const int rc = multi_ ? vr_hip_multi_set_preintegration(multi_, on ? 1u : 0u) : vr_hip_set_preintegration(ctx_, on ? 1u : 0u);
	return rc == 0 ? 0 : 1;
}

int HipRenderer::render_volume(uchar4 *buffer, Raycaster r) {
	if (!ok() || buffer == nullptr)
		return 1;
	vr_params p;
	to_params(r, sampling_, &p);
	int rc;
	mirror_error_ = nullptr;
	if (mip_ && multi_) {
		mirror_error_ = "the maximum-intensity projection renders on a single device (vr_hip_render_mip): construct the renderer without a device list";
		return 1;
	}
	if (iso_ && multi_) {
		mirror_error_ = "the isosurface renders on a single device (vr_hip_render_iso): construct the renderer without a device list";
		return 1;
	}
	if (hybrid_ && multi_) {
		mirror_error_ = "the hybrid renders on a single device (vr_hip_render_hybrid): construct the renderer without a device list";
		return 1;
	}
	if (section_ && multi_) {
		mirror_error_ = "a section frame renders on a single device (vr_hip_render_section): construct the renderer without a device list";
		return 1;
	}
	if (labelled_ && multi_) {
		mirror_error_ = "a labelled frame renders on a single device (vr_hip_render_labelled): construct the renderer without a device list";
		return 1;
	}
	if (labelled_) rc = device_buffer_ ? vr_hip_render_labelled_device(ctx_, &p, buffer, nullptr) : vr_hip_render_labelled(ctx_, &p, (uint8_t *) buffer);
	else if (section_ && section_in_volume_) rc = device_buffer_ ? vr_hip_render_section_in_volume_device(ctx_, &p, &section_params_, buffer, nullptr, nullptr) : vr_hip_render_section_in_volume(ctx_, &p, &section_params_, (uint8_t *) buffer, nullptr);
	else if (section_) rc = device_buffer_ ? vr_hip_render_section_device(ctx_, &p, &section_params_, buffer, nullptr, nullptr) : vr_hip_render_section(ctx_, &p, &section_params_, (uint8_t *) buffer, nullptr);
	else if (hybrid_) rc = device_buffer_ ? vr_hip_render_hybrid_device(ctx_, &p, &iso_params_, buffer, nullptr, nullptr) : vr_hip_render_hybrid(ctx_, &p, &iso_params_, (uint8_t *) buffer, nullptr);
	else if (iso_) rc = device_buffer_ ? vr_hip_render_iso_device(ctx_, &p, &iso_params_, buffer, nullptr, nullptr) : vr_hip_render_iso(ctx_, &p, &iso_params_, (uint8_t *) buffer, nullptr);
	else if (mip_) rc = device_buffer_ ? vr_hip_render_mip_device(ctx_, &p, buffer, nullptr) : vr_hip_render_mip(ctx_, &p, (uint8_t *) buffer);
	else if (multi_) rc = device_buffer_ ? vr_hip_multi_render_device(multi_, &p, buffer) : vr_hip_multi_render(multi_, &p, (uint8_t *) buffer);
	else rc = device_buffer_ ? vr_hip_render_device(ctx_, &p, buffer, nullptr) : vr_hip_render(ctx_, &p, (uint8_t *) buffer);
	return rc == 0 ? 0 : 1;
}

int HipRenderer::render_backdrop(uchar4 *buffer, Raycaster r, const vr_backdrop *layer) {
	if (!ok() || buffer == nullptr)
		return 1;
	mirror_error_ = nullptr;
	if (multi_) {
		mirror_error_ = "a backdrop frame renders on a single device (vr_hip_render_backdrop): construct the renderer without a device list";
		return 1;
	}
	vr_params p;
	to_params(r, sampling_, &p);
	const int rc = device_buffer_ ? vr_hip_render_backdrop_device(ctx_, &p, layer, buffer, nullptr) : vr_hip_render_backdrop(ctx_, &p, layer, (uint8_t *) buffer);
	return rc == 0 ? 0 : 1;
}

int HipRenderer::set_labels(const uint8_t *labels, const uint32_t dims[3]) {
	if (!ok())
		return 1;
	mirror_error_ = nullptr;
	if (multi_) {
		mirror_error_ = "label volumes belong to a single device (vr_hip_set_labels): construct the renderer without a device list";
		return 1;
	}
	return vr_hip_set_labels(ctx_, labels, dims ? dims[0] : 0u, dims ? dims[1] : 0u, dims ? dims[2] : 0u) == 0 ? 0 : 1;
}

int HipRenderer::set_label_table(const vr_label_entry *entries, uint32_t count) {
	if (!ok())
		return 1;
	mirror_error_ = nullptr;
	if (multi_) {
		mirror_error_ = "label tables belong to a single device (vr_hip_set_label_table): construct the renderer without a device list";
		return 1;
	}
	return vr_hip_set_label_table(ctx_, entries, count) == 0 ? 0 : 1;
}

int HipRenderer::render_depth(Raycaster r, const vr_depth &depth, const vr_depth_out *out) {
	if (!ok() || out == nullptr)
		return 1;
	mirror_error_ = nullptr;
	if (multi_) {
		mirror_error_ = "a depth frame renders on a single device (vr_hip_render_depth): construct the renderer without a device list";
		return 1;
	}
	vr_params p;
	to_params(r, sampling_, &p);
	const int rc = device_buffer_ ? vr_hip_render_depth_device(ctx_, &p, &depth, out, nullptr) : vr_hip_render_depth(ctx_, &p, &depth, out);
	return rc == 0 ? 0 : 1;
}

int HipRenderer::pick(Raycaster r, const vr_depth &depth, uint32_t n, const uint32_t *xy, vr_pick *out) {
	if (!ok())
		return 1;
	mirror_error_ = nullptr;
	if (multi_) {
		mirror_error_ = "a pick renders on a single device (vr_hip_pick): construct the renderer without a device list";
		return 1;
	}
	vr_params p;
	to_params(r, sampling_, &p);
	return vr_hip_pick(ctx_, &p, &depth, n, xy, out) == 0 ? 0 : 1;
}

}  // namespace volr
