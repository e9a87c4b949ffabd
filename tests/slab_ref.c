/*
 * slab_ref.c — the pre-integrated (slab) classification of include/vr_hip.h (vr_hip_set_preintegration) restated with the CPU oracle's own
 * statics: the composite frame whose samples take the mean of the piecewise-linear transfer function between the previous sample's
 * coordinate and their own, from the integral table K, in place of one lookup.
 * TEST INFRASTRUCTURE: compiled on demand by tests/slab_helpers.py with the flags oracle/Makefile uses for libvr_oracle.so.
 *
 * It includes tests/light_ref.c, and through it tests/shadow_ref.c and oracle/vr_oracle.c, read-only: clip_segment, scene_of, shadow_factor
 * and the arithmetic of the lighting steps are those restatements'.  slab_render_ray is light_render_ray (with a lighting) or
 * shadow_render_ray (without: the reference's cue) with the looked-up colour replaced; with slab = 0 it is those two, which
 * tests/test_slab_model.py holds it to byte for byte.
 *
 * Whole frames only (pixel (x, y) of the view -> out[y * out_width + x]).  lighting NULL = the reference's cue (light_kd); q NULL = no
 * shadow.  mode: 0 = point classification, 1 = slab classification, 2 = slab classification with the wide-slab branch in double
 * precision (K, K(t), the difference and the division; rounded to fp32 once) — what the fp32 branch is held against; 3 = a wrong reading for
 * the sensitivity tests: a sample that the library may skip without resolving it — its value below the largest power of two P whose
 * coordinate lies within the transfer function's leading zeros, behind a predecessor within them too — counts as no predecessor at all
 * for the next sample (tp = tb), instead of handing its coordinate on.  Per ray: what a wave of the library skips is a subset of it.
 * counters_out[3]: samples of the accumulation loop, those that took the wide-slab branch, those that took the narrow one.
 */
#include "light_ref.c"

#define SLAB_TF_MAX ((float) (VR_TF_SIZE - 1))

/* K[0] = 0, K[i + 1] = fmaf(0.5f, tf[i] + tf[i + 1], K[i]) per channel, in that order; K: 128 x float4 */
void slab_build_integral(const float *tf, float *K) {
	for (int ch = 0; ch < 4; ch++) {
		K[ch] = 0.0f;
		for (int i = 0; i + 1 < VR_TF_SIZE; i++)
			K[4 * (i + 1) + ch] = fmaf(0.5f, tf[4 * i + ch] + tf[4 * (i + 1) + ch], K[4 * i + ch]);
	}
}

static void slab_build_integral_double(const float *tf, double *K) {
	for (int ch = 0; ch < 4; ch++) {
		K[ch] = 0.0;
		for (int i = 0; i + 1 < VR_TF_SIZE; i++)
			K[4 * (i + 1) + ch] = K[4 * i + ch] + 0.5 * ((double) tf[4 * i + ch] + (double) tf[4 * (i + 1) + ch]);
	}
}

/* K(t), t in [0, 127] */
static f4 slab_integral_at(const float *tf, const float *K, float t) {
	uint32_t i = (uint32_t) t;
	if (i > VR_TF_SIZE - 2) i = VR_TF_SIZE - 2;
	const float w = t - (float) i;
	float r[4];
	for (int ch = 0; ch < 4; ch++)
		r[ch] = fmaf(w, fmaf(0.5f * w, tf[4 * (i + 1) + ch] - tf[4 * i + ch], tf[4 * i + ch]), K[4 * i + ch]);
	const f4 out = { r[0], r[1], r[2], r[3] };
	return out;
}

static void slab_integral_at_double(const float *tf, const double *K, float t, double *r) {
	uint32_t i = (uint32_t) t;
	if (i > VR_TF_SIZE - 2) i = VR_TF_SIZE - 2;
	const double w = (double) t - (double) i;
	for (int ch = 0; ch < 4; ch++)
		r[ch] = K[4 * i + ch] + w * ((double) tf[4 * i + ch] + 0.5 * w * ((double) tf[4 * (i + 1) + ch] - (double) tf[4 * i + ch]));
}

/* the ordinary filtered lookup of the frame's sampling mode at the coordinate t in [0, 127] */
static f4 slab_lookup(const scene *s, float t) {
	const float fl = floorf(t);
	float w = t - fl;
	if (s->p->sampling == VR_SAMPLE_TRILINEAR_Q8)
		w = rintf(w * 256.0f) * (1.0f / 256.0f);
	const uint32_t i = (uint32_t) fl, j = i + 1 < VR_TF_SIZE ? i + 1 : VR_TF_SIZE - 1;
	const f4 c0 = s->tf[i], c1 = s->tf[j];
	const f4 r = { lerp(c0.x, c1.x, w), lerp(c0.y, c1.y, w), lerp(c0.z, c1.z, w), lerp(c0.w, c1.w, w) };
	return r;
}

static void slab_render_ray(const scene *s, const float *K, const double *Kd, const float *clip, const float *lighting, uint32_t shin,
                            const uint8_t *q, uint32_t S, float strength, uint32_t mode, float skip_below, float zero_below, int px, int py,
                            uint8_t *out_px, uint64_t *samples, uint64_t *wide, uint64_t *narrow) {
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
	const float tf_scale = s->bpv == 1 ? (float) VR_TF_SIZE / 255.0f : (float) VR_TF_SIZE / 65535.0f;
	const float *tf = (const float *) s->tf;
	int first = 1, skipped = 0;
	float tp = 0.0f;
	while (kx <= ky) {
		const float xb = fmaf(kx, A.x, B.x), yb = fmaf(kx, A.y, B.y), zb = fmaf(kx, A.z, B.z);
		const float raw = sample_trilinear_raw(s, xb, yb, zb);
		f4 cur;
		(*samples)++;
		if (mode == 0)
			cur = tf_linear(s, raw);
		else {
			float tb = fmaf(raw, tf_scale, -0.5f);
			tb = tb < 0.0f ? 0.0f : (tb > SLAB_TF_MAX ? SLAB_TF_MAX : tb);          /* fmed3(.., 0, 127) for the finite coordinate of a frame */
			if (first) tp = tb;                                                     /* the loop's first sample */
			first = 0;
			if (mode == 3) {                                                        /* the wrong reading: a skipped predecessor is none */
				if (skipped) tp = tb;
				skipped = raw < skip_below && tp <= zero_below;
			}
			const float d = tb - tp;
			if (!(fabsf(d) >= 0.5f)) {                                              /* narrow slab: the lookup at its middle */
				(*narrow)++;
				cur = slab_lookup(s, 0.5f * (tp + tb));
			} else if (mode == 2) {
				(*wide)++;
				double kb[4], kp[4];
				slab_integral_at_double(tf, Kd, tb, kb);
				slab_integral_at_double(tf, Kd, tp, kp);
				const double dd = (double) tb - (double) tp;
				cur.x = (float) ((kb[0] - kp[0]) / dd); cur.y = (float) ((kb[1] - kp[1]) / dd);
				cur.z = (float) ((kb[2] - kp[2]) / dd); cur.w = (float) ((kb[3] - kp[3]) / dd);
			} else {                                                                /* wide slab: the mean of the transfer function over it */
				(*wide)++;
				const float r = 1.0f / d;
				const f4 kb = slab_integral_at(tf, K, tb), kp = slab_integral_at(tf, K, tp);
				cur.x = (kb.x - kp.x) * r; cur.y = (kb.y - kp.y) * r; cur.z = (kb.z - kp.z) * r; cur.w = (kb.w - kp.w) * r;
			}
			tp = tb;
		}
		/* everything below sees this colour and is light_render_ray's (a lighting) or shadow_render_ray's (the cue) */
		if (cur.w > 0.05f && lighting != NULL) {
			const float ka = lighting[0], kd = lighting[1], ks = lighting[2];
			const float gx = (sample_trilinear_raw(s, xb + 1.0f, yb, zb) - sample_trilinear_raw(s, xb - 1.0f, yb, zb)) * half.x;
			const float gy = (sample_trilinear_raw(s, xb, yb + 1.0f, zb) - sample_trilinear_raw(s, xb, yb - 1.0f, zb)) * half.y;
			const float gz = (sample_trilinear_raw(s, xb, yb, zb + 1.0f) - sample_trilinear_raw(s, xb, yb, zb - 1.0f)) * half.z;
			const float gg = fmaf(gz, gz, fmaf(gy, gy, gx * gx));
			if (gg > 0.0f) {
				const float ig = rsqrt_nr(gg);
				const f3 dl = f3_sub(light_pos, pt);
				const float ll = fmaf(dl.z, dl.z, fmaf(dl.y, dl.y, dl.x * dl.x));
				float sd = 0.0f, sp = 0.0f;
				if (ll > 0.0f) {
					const float il = rsqrt_nr(ll);
					const float dot = fmaf(gz, dl.z, fmaf(gy, dl.y, gx * dl.x));
					sd = fminf(fabsf((dot * ig) * il), 1.0f);
					const float iv = rsqrt_nr(fmaf(direction.z, direction.z, fmaf(direction.y, direction.y, direction.x * direction.x)));
					const f3 h = f3_make(fmaf(-direction.x, iv, dl.x * il), fmaf(-direction.y, iv, dl.y * il), fmaf(-direction.z, iv, dl.z * il));
					const float hh = fmaf(h.z, h.z, fmaf(h.y, h.y, h.x * h.x));
					if (hh > 0.0f) {
						sp = fminf(fabsf((fmaf(gz, h.z, fmaf(gy, h.y, gx * h.x)) * ig) * rsqrt_nr(hh)), 1.0f);
						for (uint32_t r = 0; r < shin; r++)
							sp = sp * sp;
					}
				}
				const float m = fmaf(kd, sd, ka);
				const float spec = (ks * sp) * cur.w;
				cur.x = fmaf(cur.x, m, spec); cur.y = fmaf(cur.y, m, spec); cur.z = fmaf(cur.z, m, spec);
			}
		} else if (cur.w > 0.05f && p->light_kd > 0.01f) {
			const f3 d = f3_sub(light_pos, pt);
			const float inv = rsqrt_nr(fmaf(d.z, d.z, fmaf(d.y, d.y, d.x * d.x)));
			const f3 light_dir = f3_scale(d, inv);
			const float raw_l = sample_trilinear_raw(s, fmaf(light_dir.x, 0.01f * half.x, xb), fmaf(light_dir.y, 0.01f * half.y, yb),
			                                         fmaf(light_dir.z, 0.01f * half.z, zb));
			const float diffuse = (raw_l - raw) * (p->light_kd * (s->bpv == 1 ? (1.0f / 255.0f) : (1.0f / 65535.0f)));
			cur.x += diffuse; cur.y += diffuse; cur.z += diffuse;
		}
		if (q != NULL && cur.w > 0.05f) {
			const float f = shadow_factor(q, S, strength, pt);
			cur.x *= f; cur.y *= f; cur.z *= f;
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

int slab_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl,
                const float *clip, const float *lighting, uint32_t shin, const uint8_t *q, uint32_t S, float strength, uint32_t mode,
                uint8_t *out, uint64_t *counters_out) {
	if ((p->sampling != VR_SAMPLE_TRILINEAR && p->sampling != VR_SAMPLE_TRILINEAR_Q8) || mode > 3)
		return 1;
	const scene s = scene_of(p, voxels, dims, bpv, tf, esl);
	float K[4 * VR_TF_SIZE];
	double Kd[4 * VR_TF_SIZE];
	slab_build_integral(tf, K);
	slab_build_integral_double(tf, Kd);
	memset(out, 0, (size_t) p->out_width * p->out_rows * 4);
	uint64_t samples = 0, wide = 0, narrow = 0;
	/* mode 3: the leading all-zero entries of the transfer function and the bound on a skippable raw value, as the library forms them */
	int zero = -1;
	while (zero + 1 < VR_TF_SIZE && tf[4 * (zero + 1)] == 0.0f && tf[4 * (zero + 1) + 1] == 0.0f && tf[4 * (zero + 1) + 2] == 0.0f && tf[4 * (zero + 1) + 3] == 0.0f)
		zero++;
	const float tf_scale = bpv == 1 ? (float) VR_TF_SIZE / 255.0f : (float) VR_TF_SIZE / 65535.0f;
	uint32_t below = 0;
	for (uint32_t P = 1; P <= (bpv == 1 ? 256u : 65536u); P <<= 1)
		if (zero >= 0 && fmaf((float) P, tf_scale, -0.5f) <= (float) zero) below = P;
	#pragma omp parallel for schedule(dynamic, 4) reduction(+:samples, wide, narrow)
	for (uint32_t y = 0; y < p->out_rows; y++)
		for (uint32_t x = 0; x < p->out_width; x++)
			slab_render_ray(&s, K, Kd, clip, lighting, shin, q, S, strength, mode, (float) below, (float) zero, (int) x, (int) y, out + ((size_t) y * p->out_width + x) * 4,
			                &samples, &wide, &narrow);
	counters_out[0] = samples; counters_out[1] = wide; counters_out[2] = narrow;
	return 0;
}
