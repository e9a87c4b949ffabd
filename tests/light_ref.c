/*
 * light_ref.c — the gradient lighting of include/vr_hip.h (vr_hip_set_lighting) restated with the CPU oracle's own statics: the composite
 * frame whose dense samples take a Blinn-Phong term from the central-difference gradient of the interpolated field in place of the
 * reference's cue, and the factor of a light grid behind it.
 * TEST INFRASTRUCTURE: compiled on demand by tests/light_helpers.py with the flags oracle/Makefile uses for libvr_oracle.so.
 *
 * It includes tests/shadow_ref.c, and through it oracle/vr_oracle.c, read-only: clip_segment, scene_of and shadow_factor are the statics of
 * that restatement, not copies.  light_render_ray is shadow_render_ray with the cue block replaced by steps 1-4 of the contract; the gradient
 * is step 6 of tests/iso_ref.c.  tests/test_light_model.py ties it to the pinned clipped composite: { 1, 0, 0, n } must give the bytes of
 * clip_render with light_kd = 0.
 *
 * Whole frames only (pixel (x, y) of the view -> out[y * out_width + x]).  lighting: ambient, diffuse, specular; shin: shininess_log2.
 * q NULL = no shadow.  counters_out[2]: dense samples (c.w > 0.05f) that were composited, and those among them with !(gg > 0).
 */
#include "shadow_ref.c"

static void light_render_ray(const scene *s, const float *clip, const float *lighting, uint32_t shin, const uint8_t *q, uint32_t S, float strength,
                             int px, int py, uint8_t *out_px, uint64_t *dense, uint64_t *flat) {
	const vr_params *p = s->p;
	f3 origin, direction;
	float kx, ky;
	get_ray(&p->view, px, py, &origin, &direction);
	if (!intersect(s, origin, direction, &kx, &ky))
		return;
	if (!clip_segment(clip, origin, direction, &kx, &ky))
		return;
	f3 pt = march_point(1, origin, direction, kx);
	while (kx <= ky) {
		if (p->esl && sample_data_esl(s, pt))
			leap_empty_space(s, pt, direction, &kx);
		else
			break;
		kx += p->ray_step;
		pt = march_point(1, origin, direction, kx);
	}
	if (kx > ky)
		return;
	f4 acc = { 0, 0, 0, 0 };
	const f3 half = f3_make(0.5f * (float) s->dx, 0.5f * (float) s->dy, 0.5f * (float) s->dz);
	const f3 A = f3_make(direction.x * half.x, direction.y * half.y, direction.z * half.z);
	const f3 B = f3_make(fmaf(origin.x, half.x, half.x - 0.5f), fmaf(origin.y, half.y, half.y - 0.5f), fmaf(origin.z, half.z, half.z - 0.5f));
	const f3 light_pos = f3_make(p->view.light_pos[0], p->view.light_pos[1], p->view.light_pos[2]);
	const float ka = lighting[0], kd = lighting[1], ks = lighting[2];
	while (kx <= ky) {
		const float xb = fmaf(kx, A.x, B.x), yb = fmaf(kx, A.y, B.y), zb = fmaf(kx, A.z, B.z);
		const float raw = sample_trilinear_raw(s, xb, yb, zb);
		f4 cur = tf_linear(s, raw);
		if (cur.w > 0.05f) {                                         /* light_kd is ignored: the cue gives way to steps 1-4 */
			(*dense)++;
			/* 1. the isosurface's gradient */
			const float gx = (sample_trilinear_raw(s, xb + 1.0f, yb, zb) - sample_trilinear_raw(s, xb - 1.0f, yb, zb)) * half.x;
			const float gy = (sample_trilinear_raw(s, xb, yb + 1.0f, zb) - sample_trilinear_raw(s, xb, yb - 1.0f, zb)) * half.y;
			const float gz = (sample_trilinear_raw(s, xb, yb, zb + 1.0f) - sample_trilinear_raw(s, xb, yb, zb - 1.0f)) * half.z;
			const float gg = fmaf(gz, gz, fmaf(gy, gy, gx * gx));
			if (gg > 0.0f) {
				/* 2. light */
				const float ig = rsqrt_nr(gg);
				const f3 dl = f3_sub(light_pos, pt);
				const float ll = fmaf(dl.z, dl.z, fmaf(dl.y, dl.y, dl.x * dl.x));
				float sd = 0.0f, sp = 0.0f;
				if (ll > 0.0f) {
					const float il = rsqrt_nr(ll);
					const float dot = fmaf(gz, dl.z, fmaf(gy, dl.y, gx * dl.x));
					sd = fminf(fabsf((dot * ig) * il), 1.0f);
					/* 3. highlight */
					const float iv = rsqrt_nr(fmaf(direction.z, direction.z, fmaf(direction.y, direction.y, direction.x * direction.x)));
					const f3 h = f3_make(fmaf(-direction.x, iv, dl.x * il), fmaf(-direction.y, iv, dl.y * il), fmaf(-direction.z, iv, dl.z * il));
					const float hh = fmaf(h.z, h.z, fmaf(h.y, h.y, h.x * h.x));
					if (hh > 0.0f) {
						sp = fminf(fabsf((fmaf(gz, h.z, fmaf(gy, h.y, gx * h.x)) * ig) * rsqrt_nr(hh)), 1.0f);
						for (uint32_t r = 0; r < shin; r++)
							sp = sp * sp;
					}
				}
				/* 4. colour; cur.w is untouched */
				const float m = fmaf(kd, sd, ka);
				const float spec = (ks * sp) * cur.w;
				cur.x = fmaf(cur.x, m, spec); cur.y = fmaf(cur.y, m, spec); cur.z = fmaf(cur.z, m, spec);
			} else
				(*flat)++;
			if (q != NULL) {                                         /* 5. the shadow's factor, after step 4 */
				const float f = shadow_factor(q, S, strength, pt);
				cur.x *= f; cur.y *= f; cur.z *= f;
			}
		}
		const float t = 1 - acc.w;
		acc.x = fmaf(cur.x, t, acc.x); acc.y = fmaf(cur.y, t, acc.y);
		acc.z = fmaf(cur.z, t, acc.z); acc.w = fmaf(cur.w, t, acc.w);
		if (acc.w > p->ray_threshold)
			break;
		kx += p->ray_step;
		pt = march_point(1, origin, direction, kx);
	}
	out_px[0] = (uint8_t) map_float_int(acc.x, 256);
	out_px[1] = (uint8_t) map_float_int(acc.y, 256);
	out_px[2] = (uint8_t) map_float_int(acc.z, 256);
	out_px[3] = (uint8_t) map_float_int(acc.w, 256);
}

int light_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl,
                 const float *clip, const float *lighting, uint32_t shin, const uint8_t *q, uint32_t S, float strength, uint8_t *out,
                 uint64_t *counters_out) {
	if (p->sampling != VR_SAMPLE_TRILINEAR && p->sampling != VR_SAMPLE_TRILINEAR_Q8)
		return 1;
	const scene s = scene_of(p, voxels, dims, bpv, tf, esl);
	memset(out, 0, (size_t) p->out_width * p->out_rows * 4);
	uint64_t dense = 0, flat = 0;
	#pragma omp parallel for schedule(dynamic, 4) reduction(+:dense, flat)
	for (uint32_t y = 0; y < p->out_rows; y++)
		for (uint32_t x = 0; x < p->out_width; x++)
			light_render_ray(&s, clip, lighting, shin, q, S, strength, (int) x, (int) y, out + ((size_t) y * p->out_width + x) * 4, &dense, &flat);
	counters_out[0] = dense; counters_out[1] = flat;
	return 0;
}
