/*
 * clip_ref.c — the clip region of include/vr_hip.h (vr_hip_set_clip) restated with the CPU oracle's own statics, for all three projections.
 * TEST INFRASTRUCTURE: compiled on demand by tests/clip_helpers.py with the flags oracle/Makefile uses for libvr_oracle.so.
 *
 * It includes oracle/vr_oracle.c read-only.  Each renderer is the pinned restatement of its projection — render_ray of vr_oracle.c,
 * the loop of tests/mip_ref.c, the loop of tests/iso_ref.c (without the skipping emulation: skipping never changes a frame) — with steps
 * 1-3 of the clip contract (clip_segment below) between intersect and the march, and nothing else changed.  tests/test_clip_model.py ties
 * them to those restatements: with the box [-1,1]^3 and no plane they must give the same bytes.
 *
 * Whole frames only (pixel (x, y) of the view -> out[y * out_width + x]).  clip: box_min[3], box_max[3], plane[4] as in vr_clip.
 */
#include "../oracle/vr_oracle.c"

/* steps 1-3 of the contract; returns the hit test on the narrowed segment */
static int clip_segment(const float *clip, f3 o, f3 dir, float *kx, float *ky) {
	f3 d = dir;
	if (d.x == 0) d.x = 0.00001f;
	if (d.y == 0) d.y = 0.00001f;
	if (d.z == 0) d.z = 0.00001f;
	const f3 k1 = f3_div(f3_sub(f3_make(clip[0], clip[1], clip[2]), o), d);
	const f3 k2 = f3_div(f3_sub(f3_make(clip[3], clip[4], clip[5]), o), d);
	const float kxb = flmax(flmax(flmin(k1.x, k2.x), flmin(k1.y, k2.y)), flmin(k1.z, k2.z));
	const float kyb = flmin(flmin(flmax(k1.x, k2.x), flmax(k1.y, k2.y)), flmax(k1.z, k2.z));
	*kx = flmax(*kx, kxb);
	*ky = flmin(*ky, kyb);
	const float *n = clip + 6;
	const float dn = fmaf(n[2], dir.z, fmaf(n[1], dir.y, n[0] * dir.x));
	const float on = fmaf(n[2], o.z, fmaf(n[1], o.y, fmaf(n[0], o.x, n[3])));
	if (dn > 0) *kx = flmax(*kx, -on / dn);
	else if (dn < 0) *ky = flmin(*ky, -on / dn);
	else if (!(on >= 0)) return 0;
	return (*kx < *ky) && (*ky > 0);
}

static scene scene_of(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl) {
	scene s;
	s.p = p; s.vox8 = (const uint8_t *) voxels; s.vox16 = (const uint16_t *) voxels;
	s.dx = dims[0]; s.dy = dims[1]; s.dz = dims[2]; s.bpv = bpv;
	s.tf = (const f4 *) tf; s.esl = esl; s.min_bound = f3_make(-1, -1, -1); s.line_bits = NULL;
	return s;
}

/* render_ray of oracle/vr_oracle.c (NEAREST and the TRILINEAR modes), the segment clipped */
static void clip_render_ray(const scene *s, const float *clip, int px, int py, uint8_t *out_px) {
	const vr_params *p = s->p;
	f3 origin, direction;
	float kx, ky;
	get_ray(&p->view, px, py, &origin, &direction);
	if (!intersect(s, origin, direction, &kx, &ky))
		return;
	if (!clip_segment(clip, origin, direction, &kx, &ky))
		return;
	const int fused = p->sampling != VR_SAMPLE_NEAREST;
	f3 pt = march_point(fused, origin, direction, kx);
	while (kx <= ky) {
		if (p->esl && sample_data_esl(s, pt))
			leap_empty_space(s, pt, direction, &kx);
		else
			break;
		kx += p->ray_step;
		pt = march_point(fused, origin, direction, kx);
	}
	if (kx > ky)
		return;
	f4 acc = { 0, 0, 0, 0 };
	const f3 half = f3_make(0.5f * (float) s->dx, 0.5f * (float) s->dy, 0.5f * (float) s->dz);
	const f3 A = f3_make(direction.x * half.x, direction.y * half.y, direction.z * half.z);
	const f3 B = f3_make(fmaf(origin.x, half.x, half.x - 0.5f), fmaf(origin.y, half.y, half.y - 0.5f), fmaf(origin.z, half.z, half.z - 0.5f));
	const f3 light_pos = f3_make(p->view.light_pos[0], p->view.light_pos[1], p->view.light_pos[2]);
	const float raw_scale = s->bpv == 1 ? 255.0f : 65535.0f;
	while (kx <= ky) {
		f4 cur;
		if (!fused) {
			const uint32_t sample = sample_nearest(s, pt);
			const uint32_t s8 = s->bpv == 1 ? sample : (sample >> 8);
			cur = s->tf[s8 / VR_TF_RATIO];
			if (cur.w > 0.05f && p->light_kd > 0.01f) {
				const f3 light_dir = vector_normalize(f3_sub(light_pos, pt));
				const float sample_l = (float) sample_nearest(s, f3_add(pt, f3_scale(light_dir, 0.01f))) / raw_scale;
				const float diffuse = (sample_l - (float) sample / raw_scale) * p->light_kd;
				cur.x += diffuse; cur.y += diffuse; cur.z += diffuse;
			}
		} else {
			const float xb = fmaf(kx, A.x, B.x), yb = fmaf(kx, A.y, B.y), zb = fmaf(kx, A.z, B.z);
			const float raw = sample_trilinear_raw(s, xb, yb, zb);
			cur = tf_linear(s, raw);
			if (cur.w > 0.05f && p->light_kd > 0.01f) {
				const f3 d = f3_sub(light_pos, pt);
				const float inv = rsqrt_nr(fmaf(d.z, d.z, fmaf(d.y, d.y, d.x * d.x)));
				const f3 light_dir = f3_scale(d, inv);
				const float raw_l = sample_trilinear_raw(s, fmaf(light_dir.x, 0.01f * half.x, xb), fmaf(light_dir.y, 0.01f * half.y, yb),
				                                         fmaf(light_dir.z, 0.01f * half.z, zb));
				const float diffuse = (raw_l - raw) * (p->light_kd * (s->bpv == 1 ? (1.0f / 255.0f) : (1.0f / 65535.0f)));
				cur.x += diffuse; cur.y += diffuse; cur.z += diffuse;
			}
		}
		const float t = 1 - acc.w;
		if (fused) {
			acc.x = fmaf(cur.x, t, acc.x); acc.y = fmaf(cur.y, t, acc.y);
			acc.z = fmaf(cur.z, t, acc.z); acc.w = fmaf(cur.w, t, acc.w);
		} else {
			acc.x = acc.x + cur.x * t; acc.y = acc.y + cur.y * t;
			acc.z = acc.z + cur.z * t; acc.w = acc.w + cur.w * t;
		}
		if (acc.w > p->ray_threshold)
			break;
		kx += p->ray_step;
		pt = march_point(fused, origin, direction, kx);
	}
	out_px[0] = (uint8_t) map_float_int(acc.x, 256);
	out_px[1] = (uint8_t) map_float_int(acc.y, 256);
	out_px[2] = (uint8_t) map_float_int(acc.z, 256);
	out_px[3] = (uint8_t) map_float_int(acc.w, 256);
}

int clip_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl,
                const float *clip, uint8_t *out) {
	const scene s = scene_of(p, voxels, dims, bpv, tf, esl);
	memset(out, 0, (size_t) p->out_width * p->out_rows * 4);
	#pragma omp parallel for schedule(dynamic, 4)
	for (uint32_t y = 0; y < p->out_rows; y++)
		for (uint32_t x = 0; x < p->out_width; x++)
			clip_render_ray(&s, clip, (int) x, (int) y, out + ((size_t) y * p->out_width + x) * 4);
	return 0;
}

/* mip_render of tests/mip_ref.c, the segment clipped */
int clip_mip_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const float *clip, uint8_t *out) {
	const scene s = scene_of(p, voxels, dims, bpv, tf, NULL);
	memset(out, 0, (size_t) p->out_width * p->out_rows * 4);
	#pragma omp parallel for schedule(dynamic, 4)
	for (uint32_t y = 0; y < p->out_rows; y++)
		for (uint32_t x = 0; x < p->out_width; x++) {
			f3 o, d;
			float kx, ky;
			const size_t px = (size_t) y * p->out_width + x;
			get_ray(&p->view, (int) x, (int) y, &o, &d);
			if (!intersect(&s, o, d, &kx, &ky))
				continue;
			if (!clip_segment(clip, o, d, &kx, &ky))
				continue;
			const int fused = p->sampling != VR_SAMPLE_NEAREST;
			const f3 half = f3_make(0.5f * (float) s.dx, 0.5f * (float) s.dy, 0.5f * (float) s.dz);
			const f3 A = f3_make(d.x * half.x, d.y * half.y, d.z * half.z);
			const f3 B = f3_make(fmaf(o.x, half.x, half.x - 0.5f), fmaf(o.y, half.y, half.y - 0.5f), fmaf(o.z, half.z, half.z - 0.5f));
			uint32_t mi = 0;
			float mf = 0.0f;
			while (kx <= ky) {
				if (!fused) {
					const uint32_t v = sample_nearest(&s, march_point(0, o, d, kx));
					if (v > mi) mi = v;
				} else {
					const float r = sample_trilinear_raw(&s, fmaf(kx, A.x, B.x), fmaf(kx, A.y, B.y), fmaf(kx, A.z, B.z));
					if (r > mf) mf = r;
				}
				kx += p->ray_step;
			}
			f4 c;
			if (!fused) {
				const uint32_t s8 = bpv == 1 ? mi : mi >> 8;
				c = s.tf[s8 / VR_TF_RATIO];
			} else {
				c = tf_linear(&s, mf);
			}
			out[4 * px + 0] = (uint8_t) map_float_int(c.x, 256); out[4 * px + 1] = (uint8_t) map_float_int(c.y, 256);
			out[4 * px + 2] = (uint8_t) map_float_int(c.z, 256); out[4 * px + 3] = (uint8_t) map_float_int(c.w, 256);
		}
	return 0;
}

/* iso_render of tests/iso_ref.c, the segment clipped; ray_out (may be NULL): origin and direction of every pixel's ray, six floats */
int clip_iso_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, float level, uint32_t refine,
                    const float *clip, uint8_t *out, float *depth_out, float *ray_out) {
	if (p->sampling != VR_SAMPLE_TRILINEAR && p->sampling != VR_SAMPLE_TRILINEAR_Q8)
		return 1;
	const scene s = scene_of(p, voxels, dims, bpv, tf, NULL);
	const f3 half = f3_make(0.5f * (float) s.dx, 0.5f * (float) s.dy, 0.5f * (float) s.dz);
	const f3 light_pos = f3_make(p->view.light_pos[0], p->view.light_pos[1], p->view.light_pos[2]);
	const f4 base = tf_linear(&s, level);
	memset(out, 0, (size_t) p->out_width * p->out_rows * 4);
	#pragma omp parallel for schedule(dynamic, 4)
	for (uint32_t y = 0; y < p->out_rows; y++)
		for (uint32_t x = 0; x < p->out_width; x++) {
			f3 o, d;
			float kx, ky;
			const size_t px = (size_t) y * p->out_width + x;
			depth_out[px] = -1.0f;
			get_ray(&p->view, (int) x, (int) y, &o, &d);
			if (ray_out != NULL) { float *r = ray_out + 6 * px; r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z; }
			if (!intersect(&s, o, d, &kx, &ky))
				continue;
			if (!clip_segment(clip, o, d, &kx, &ky))
				continue;
			const f3 A = f3_make(d.x * half.x, d.y * half.y, d.z * half.z);
			const f3 B = f3_make(fmaf(o.x, half.x, half.x - 0.5f), fmaf(o.y, half.y, half.y - 0.5f), fmaf(o.z, half.z, half.z - 0.5f));
#define V_AT(k) sample_trilinear_raw(&s, fmaf((k), A.x, B.x), fmaf((k), A.y, B.y), fmaf((k), A.z, B.z))
			int found = 0, first = 1;
			float lo = kx, hi = kx;
			while (kx <= ky) {
				if (V_AT(kx) >= level) { found = 1; hi = kx; if (first) lo = kx; break; }
				lo = kx;
				first = 0;
				kx += p->ray_step;
			}
			if (!found)
				continue;
			if (!first)
				for (uint32_t r = 0; r < refine; r++) {
					const float mid = 0.5f * (lo + hi);
					if (V_AT(mid) >= level) hi = mid; else lo = mid;
				}
			depth_out[px] = hi;
			float f = 1.0f;
			if (!(p->light_kd <= 0.01f)) {
				const float xb = fmaf(hi, A.x, B.x), yb = fmaf(hi, A.y, B.y), zb = fmaf(hi, A.z, B.z);
				const float gx = (sample_trilinear_raw(&s, xb + 1.0f, yb, zb) - sample_trilinear_raw(&s, xb - 1.0f, yb, zb)) * half.x;
				const float gy = (sample_trilinear_raw(&s, xb, yb + 1.0f, zb) - sample_trilinear_raw(&s, xb, yb - 1.0f, zb)) * half.y;
				const float gz = (sample_trilinear_raw(&s, xb, yb, zb + 1.0f) - sample_trilinear_raw(&s, xb, yb, zb - 1.0f)) * half.z;
				const float gg = fmaf(gz, gz, fmaf(gy, gy, gx * gx));
				float sh = 0.0f;
				if (gg > 0.0f) {
					const f3 pt = march_point(1, o, d, hi);
					const f3 dl = f3_sub(light_pos, pt);
					const float il = rsqrt_nr(fmaf(dl.z, dl.z, fmaf(dl.y, dl.y, dl.x * dl.x)));
					const float dot = fmaf(gz, dl.z, fmaf(gy, dl.y, gx * dl.x));
					sh = fminf(fabsf((dot * rsqrt_nr(gg)) * il), 1.0f);
				}
				f = fmaf(p->light_kd, sh, 1.0f - p->light_kd);
			}
#undef V_AT
			out[4 * px + 0] = (uint8_t) map_float_int(base.x * f, 256); out[4 * px + 1] = (uint8_t) map_float_int(base.y * f, 256);
			out[4 * px + 2] = (uint8_t) map_float_int(base.z * f, 256); out[4 * px + 3] = (uint8_t) map_float_int(base.w, 256);
		}
	return 0;
}
