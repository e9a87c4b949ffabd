// abi_stub.cpp — a stand-alone definition of the 44 C-ABI entries (include/vr_hip.h) that the host layer calls: the mirror
// (csrc/host/HipRenderer.cpp) and the headless driver (csrc/host/volr_bench.cpp).  Linked in place of libvr_hip.so it lets
// those two run whole command lines and call sequences on a CPU; tests/test_host_layers.py holds what they print and what
// they pass down against recorded fixtures.
//
// Every entry but the two last_error queries (what they return shows in what the caller prints) appends one line to the trace:
// the file named by VR_STUB_TRACE, else stderr.  A line holds the entry's name, every scalar argument, every struct argument member by member, pointer arguments as 0 / 1 (null / non-null), and of
// vr_params the members the host layer decides (not the camera vectors: camera.cpp's arithmetic is not what is pinned here).
// Entries return 0; VR_STUB_FAIL=<entry>[:<code>] makes the first call of that entry return <code> (default 1) instead —
// a failing vr_hip_create / vr_hip_multi_create then hands back no handle.  Render entries leave the buffers alone;
// vr_hip_pick zeroes its records, because the driver prints them.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/vr_hip.h"

namespace {

FILE *trace_file() {
	static FILE *f = nullptr;
	if (f == nullptr) {
		const char *path = getenv("VR_STUB_TRACE");
		f = path != nullptr && path[0] != '\0' ? fopen(path, "a") : nullptr;
		if (f == nullptr) f = stderr;
	}
	return f;
}

void put(const char *fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vfprintf(trace_file(), fmt, ap);
	va_end(ap);
}

// ends the entry's line and decides what the entry returns
int done(const char *entry) {
	static bool failed = false;
	int rc = 0;
	const char *want = getenv("VR_STUB_FAIL");
	if (!failed && want != nullptr) {
		const size_t n = strlen(entry);
		if (strncmp(want, entry, n) == 0 && (want[n] == '\0' || want[n] == ':')) {
			rc = want[n] == ':' ? atoi(want + n + 1) : 1;
			failed = true;
		}
	}
	put(" -> %d\n", rc);
	fflush(trace_file());
	return rc;
}

int is(const void *p) { return p != nullptr ? 1 : 0; }

void put_params(const vr_params *p) {
	if (p == nullptr) { put(" params=0"); return; }
	// sampling, esl / esl_block_dims, ray_step, ray_threshold, light_kd, x0, out_width x out_rows, band_rows / band_stride / band_first, view.width x view.height, view.perspective
	put(" params{s=%u esl=%u/%u step=%.9g thr=%.9g kd=%.9g x0=%u out=%ux%u band=%u/%u/%u view=%ux%u persp=%u}", p->sampling, p->esl, p->esl_block_dims, p->ray_step,
	    p->ray_threshold, p->light_kd, p->x0, p->out_width, p->out_rows, p->band_rows, p->band_stride, p->band_first, p->view.width, p->view.height, p->view.perspective);
}

void put_iso(const vr_iso *i) {
	if (i == nullptr) { put(" iso=0"); return; }
	put(" iso{level=%.9g refine=%u}", i->level, i->refine);
}

void put_section(const vr_section *s) {
	if (s == nullptr) { put(" section=0"); return; }
	put(" section{plane=%.9g,%.9g,%.9g,%.9g half_width=%.9g mode=%u window=%.9g,%.9g}", s->plane[0], s->plane[1], s->plane[2], s->plane[3], s->half_width, s->mode,
	    s->window[0], s->window[1]);
}

void put_depth(const vr_depth *d) {
	if (d == nullptr) { put(" depth=0"); return; }
	put(" depth{opacity=%.9g mode=%u}", d->opacity, d->mode);
}

void put_depth_out(const vr_depth_out *o) {
	if (o == nullptr) { put(" out=0"); return; }
	put(" out{depth=%d value=%d alpha=%d}", is(o->depth), is(o->value), is(o->alpha));
}

void put_backdrop(const vr_backdrop *b) {
	if (b == nullptr) { put(" layer=0"); return; }
	put(" layer{rgba=%d depth=%d}", is(b->rgba), is(b->depth));
}

int handle_cell;        // what the handles point at: the host layer never looks behind them

int render(const char *entry, const void *ctx, const vr_params *p, const void *rgba) {
	put("%s ctx=%d", entry, is(ctx));
	put_params(p);
	put(" rgba=%d", is(rgba));
	return done(entry);
}

int render_on(const char *entry, const void *ctx, const vr_params *p, const void *rgba, const void *stream) {
	put("%s ctx=%d", entry, is(ctx));
	put_params(p);
	put(" rgba=%d stream=%d", is(rgba), is(stream));
	return done(entry);
}

int render_iso(const char *entry, const void *ctx, const vr_params *p, const vr_iso *iso, const void *rgba, const void *depth, int stream) {
	put("%s ctx=%d", entry, is(ctx));
	put_params(p);
	put_iso(iso);
	put(" rgba=%d depth=%d", is(rgba), is(depth));
	if (stream >= 0) put(" stream=%d", stream);
	return done(entry);
}

int render_section(const char *entry, const void *ctx, const vr_params *p, const vr_section *s, const void *rgba, const void *depth, int stream) {
	put("%s ctx=%d", entry, is(ctx));
	put_params(p);
	put_section(s);
	put(" rgba=%d depth=%d", is(rgba), is(depth));
	if (stream >= 0) put(" stream=%d", stream);
	return done(entry);
}

int set_window(const char *entry, const void *h, uint32_t w, uint32_t ht) {
	put("%s ctx=%d width=%u height=%u", entry, is(h), w, ht);
	return done(entry);
}

int set_transfer_fn(const char *entry, const void *h, const float *tf, const uint32_t *esl) {
	put("%s ctx=%d tf=%d esl=%d", entry, is(h), is(tf), is(esl));
	return done(entry);
}

int set_volume(const char *entry, const void *h, const void *v, uint32_t x, uint32_t y, uint32_t z, uint32_t bpv) {
	put("%s ctx=%d voxels=%d dims=%u,%u,%u bytes_per_voxel=%u", entry, is(h), is(v), x, y, z, bpv);
	return done(entry);
}

int set_clip(const char *entry, const void *h, const vr_clip *c) {
	put("%s ctx=%d", entry, is(h));
	if (c == nullptr) put(" clip=0");
	else put(" clip{box_min=%.9g,%.9g,%.9g box_max=%.9g,%.9g,%.9g plane=%.9g,%.9g,%.9g,%.9g}", c->box_min[0], c->box_min[1], c->box_min[2], c->box_max[0], c->box_max[1], c->box_max[2],
	         c->plane[0], c->plane[1], c->plane[2], c->plane[3]);
	return done(entry);
}

int set_shadow(const char *entry, const void *h, const vr_shadow *s) {
	put("%s ctx=%d", entry, is(h));
	if (s == nullptr) put(" shadow=0");
	else put(" shadow{light_pos=%.9g,%.9g,%.9g dims=%u step=%.9g strength=%.9g cutoff=%.9g sampling=%u}", s->light_pos[0], s->light_pos[1], s->light_pos[2], s->dims, s->step,
	         s->strength, s->cutoff, s->sampling);
	return done(entry);
}

int set_lighting(const char *entry, const void *h, const vr_lighting *l) {
	put("%s ctx=%d", entry, is(h));
	if (l == nullptr) put(" lighting=0");
	else put(" lighting{ambient=%.9g diffuse=%.9g specular=%.9g shininess_log2=%u}", l->ambient, l->diffuse, l->specular, l->shininess_log2);
	return done(entry);
}

int set_preintegration(const char *entry, const void *h, uint32_t on) {
	put("%s ctx=%d on=%u", entry, is(h), on);
	return done(entry);
}

}  // namespace

extern "C" {

int vr_hip_create(int device, vr_ctx **out) {
	put("vr_hip_create device=%d out=%d", device, is(out));
	const int rc = done("vr_hip_create");
	if (out != nullptr) *out = rc == 0 ? (vr_ctx *) &handle_cell : nullptr;
	return rc;
}
void vr_hip_destroy(vr_ctx *ctx) { put("vr_hip_destroy ctx=%d\n", is(ctx)); }
const char *vr_hip_last_error(const vr_ctx *) { return "stub: the context's error"; }

int vr_hip_set_window(vr_ctx *ctx, uint32_t w, uint32_t h) { return set_window("vr_hip_set_window", ctx, w, h); }
int vr_hip_set_transfer_fn(vr_ctx *ctx, const float *tf, const uint32_t *esl) { return set_transfer_fn("vr_hip_set_transfer_fn", ctx, tf, esl); }
int vr_hip_set_volume(vr_ctx *ctx, const void *v, uint32_t x, uint32_t y, uint32_t z, uint32_t bpv) { return set_volume("vr_hip_set_volume", ctx, v, x, y, z, bpv); }
int vr_hip_set_clip(vr_ctx *ctx, const vr_clip *clip) { return set_clip("vr_hip_set_clip", ctx, clip); }
int vr_hip_set_shadow(vr_ctx *ctx, const vr_shadow *shadow) { return set_shadow("vr_hip_set_shadow", ctx, shadow); }
int vr_hip_set_lighting(vr_ctx *ctx, const vr_lighting *lighting) { return set_lighting("vr_hip_set_lighting", ctx, lighting); }
int vr_hip_set_preintegration(vr_ctx *ctx, uint32_t on) { return set_preintegration("vr_hip_set_preintegration", ctx, on); }

int vr_hip_render(vr_ctx *ctx, const vr_params *p, uint8_t *rgba) { return render("vr_hip_render", ctx, p, rgba); }
int vr_hip_render_device(vr_ctx *ctx, const vr_params *p, void *rgba, void *stream) { return render_on("vr_hip_render_device", ctx, p, rgba, stream); }
int vr_hip_render_mip(vr_ctx *ctx, const vr_params *p, uint8_t *rgba) { return render("vr_hip_render_mip", ctx, p, rgba); }
int vr_hip_render_mip_device(vr_ctx *ctx, const vr_params *p, void *rgba, void *stream) { return render_on("vr_hip_render_mip_device", ctx, p, rgba, stream); }
int vr_hip_render_labelled(vr_ctx *ctx, const vr_params *p, uint8_t *rgba) { return render("vr_hip_render_labelled", ctx, p, rgba); }
int vr_hip_render_labelled_device(vr_ctx *ctx, const vr_params *p, void *rgba, void *stream) { return render_on("vr_hip_render_labelled_device", ctx, p, rgba, stream); }

int vr_hip_render_iso(vr_ctx *ctx, const vr_params *p, const vr_iso *iso, uint8_t *rgba, float *depth) { return render_iso("vr_hip_render_iso", ctx, p, iso, rgba, depth, -1); }
int vr_hip_render_iso_device(vr_ctx *ctx, const vr_params *p, const vr_iso *iso, void *rgba, void *depth, void *stream) {
	return render_iso("vr_hip_render_iso_device", ctx, p, iso, rgba, depth, is(stream));
}
int vr_hip_render_hybrid(vr_ctx *ctx, const vr_params *p, const vr_iso *iso, uint8_t *rgba, float *depth) { return render_iso("vr_hip_render_hybrid", ctx, p, iso, rgba, depth, -1); }
int vr_hip_render_hybrid_device(vr_ctx *ctx, const vr_params *p, const vr_iso *iso, void *rgba, void *depth, void *stream) {
	return render_iso("vr_hip_render_hybrid_device", ctx, p, iso, rgba, depth, is(stream));
}

int vr_hip_render_section(vr_ctx *ctx, const vr_params *p, const vr_section *s, uint8_t *rgba, float *depth) { return render_section("vr_hip_render_section", ctx, p, s, rgba, depth, -1); }
int vr_hip_render_section_device(vr_ctx *ctx, const vr_params *p, const vr_section *s, void *rgba, void *depth, void *stream) {
	return render_section("vr_hip_render_section_device", ctx, p, s, rgba, depth, is(stream));
}
int vr_hip_render_section_in_volume(vr_ctx *ctx, const vr_params *p, const vr_section *s, uint8_t *rgba, float *depth) {
	return render_section("vr_hip_render_section_in_volume", ctx, p, s, rgba, depth, -1);
}
int vr_hip_render_section_in_volume_device(vr_ctx *ctx, const vr_params *p, const vr_section *s, void *rgba, void *depth, void *stream) {
	return render_section("vr_hip_render_section_in_volume_device", ctx, p, s, rgba, depth, is(stream));
}

int vr_hip_render_backdrop(vr_ctx *ctx, const vr_params *p, const vr_backdrop *layer, uint8_t *rgba) {
	put("vr_hip_render_backdrop ctx=%d", is(ctx));
	put_params(p);
	put_backdrop(layer);
	put(" rgba=%d", is(rgba));
	return done("vr_hip_render_backdrop");
}
int vr_hip_render_backdrop_device(vr_ctx *ctx, const vr_params *p, const vr_backdrop *layer, void *rgba, void *stream) {
	put("vr_hip_render_backdrop_device ctx=%d", is(ctx));
	put_params(p);
	put_backdrop(layer);
	put(" rgba=%d stream=%d", is(rgba), is(stream));
	return done("vr_hip_render_backdrop_device");
}

int vr_hip_render_depth(vr_ctx *ctx, const vr_params *p, const vr_depth *d, const vr_depth_out *out) {
	put("vr_hip_render_depth ctx=%d", is(ctx));
	put_params(p);
	put_depth(d);
	put_depth_out(out);
	return done("vr_hip_render_depth");
}
int vr_hip_render_depth_device(vr_ctx *ctx, const vr_params *p, const vr_depth *d, const vr_depth_out *out, void *stream) {
	put("vr_hip_render_depth_device ctx=%d", is(ctx));
	put_params(p);
	put_depth(d);
	put_depth_out(out);
	put(" stream=%d", is(stream));
	return done("vr_hip_render_depth_device");
}
int vr_hip_pick(vr_ctx *ctx, const vr_params *p, const vr_depth *d, uint32_t n, const uint32_t *xy, vr_pick *out) {
	put("vr_hip_pick ctx=%d", is(ctx));
	put_params(p);
	put_depth(d);
	put(" n=%u xy=", n);
	if (xy == nullptr) put("0");
	else for (uint32_t i = 0; i < 2u * n; i++) put(i ? ",%u" : "%u", xy[i]);
	put(" out=%d", is(out));
	if (out != nullptr) memset(out, 0, sizeof(vr_pick) * n);
	return done("vr_hip_pick");
}

int vr_hip_set_labels(vr_ctx *ctx, const uint8_t *labels, uint32_t x, uint32_t y, uint32_t z) {
	put("vr_hip_set_labels ctx=%d labels=%d dims=%u,%u,%u", is(ctx), is(labels), x, y, z);
	return done("vr_hip_set_labels");
}
int vr_hip_set_label_table(vr_ctx *ctx, const vr_label_entry *entries, uint32_t count) {
	put("vr_hip_set_label_table ctx=%d entries=%d count=%u", is(ctx), is(entries), count);
	for (uint32_t i = 0; entries != nullptr && i < count; i++) {
		const vr_label_entry &e = entries[i];
		if (e.colour[0] != 0.0f || e.colour[1] != 0.0f || e.colour[2] != 0.0f || e.mix != 0.0f || e.opacity != 1.0f)       // the identity entries are not spelled out
			put(" [%u]{colour=%.9g,%.9g,%.9g mix=%.9g opacity=%.9g}", i, entries[i].colour[0], entries[i].colour[1], entries[i].colour[2], entries[i].mix, entries[i].opacity);
	}
	return done("vr_hip_set_label_table");
}

int vr_hip_multi_create(int n, const int *devices, vr_multi **out) {
	put("vr_hip_multi_create n=%d devices=", n);
	if (devices == nullptr) put("0");
	else for (int i = 0; i < n; i++) put(i ? ",%d" : "%d", devices[i]);
	put(" out=%d", is(out));
	const int rc = done("vr_hip_multi_create");
	if (out != nullptr) *out = rc == 0 ? (vr_multi *) &handle_cell : nullptr;
	return rc;
}
void vr_hip_multi_destroy(vr_multi *m) { put("vr_hip_multi_destroy m=%d\n", is(m)); }
const char *vr_hip_multi_last_error(const vr_multi *) { return "stub: the device list's error"; }
const char *vr_hip_multi_transport(const vr_multi *m) { put("vr_hip_multi_transport m=%d\n", is(m)); return "stub-transport"; }

int vr_hip_multi_set_window(vr_multi *m, uint32_t w, uint32_t h) { return set_window("vr_hip_multi_set_window", m, w, h); }
int vr_hip_multi_set_transfer_fn(vr_multi *m, const float *tf, const uint32_t *esl) { return set_transfer_fn("vr_hip_multi_set_transfer_fn", m, tf, esl); }
int vr_hip_multi_set_volume(vr_multi *m, const void *v, uint32_t x, uint32_t y, uint32_t z, uint32_t bpv) { return set_volume("vr_hip_multi_set_volume", m, v, x, y, z, bpv); }
int vr_hip_multi_set_clip(vr_multi *m, const vr_clip *clip) { return set_clip("vr_hip_multi_set_clip", m, clip); }
int vr_hip_multi_set_shadow(vr_multi *m, const vr_shadow *shadow) { return set_shadow("vr_hip_multi_set_shadow", m, shadow); }
int vr_hip_multi_set_lighting(vr_multi *m, const vr_lighting *lighting) { return set_lighting("vr_hip_multi_set_lighting", m, lighting); }
int vr_hip_multi_set_preintegration(vr_multi *m, uint32_t on) { return set_preintegration("vr_hip_multi_set_preintegration", m, on); }
int vr_hip_multi_render(vr_multi *m, const vr_params *p, uint8_t *rgba) { return render("vr_hip_multi_render", m, p, rgba); }
int vr_hip_multi_render_device(vr_multi *m, const vr_params *p, void *rgba) { return render("vr_hip_multi_render_device", m, p, rgba); }

}  // extern "C"
