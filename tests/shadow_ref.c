/*
 * shadow_ref.c — the light-source shadows of include/vr_hip.h (vr_hip_set_shadow) restated with the CPU oracle's own statics: the builder
 * of the light grid and the composite frame whose dense samples are scaled by it.
 * TEST INFRASTRUCTURE: compiled on demand by tests/shadow_helpers.py with the flags oracle/Makefile uses for libvr_oracle.so.
 *
 * It includes oracle/vr_oracle.c read-only.  shadow_build is steps 1-5 of the contract.  shadow_render is clip_render_ray of tests/clip_ref.c
 * (TRILINEAR modes; clip_segment is restated here with it) with the one added scaling; tests/test_shadow_model.py ties it to that
 * restatement: without a grid, and with strength 0, it must give the same bytes.
 *
 * Whole frames only (pixel (x, y) of the view -> out[y * out_width + x]).  clip: box_min[3], box_max[3], plane[4] as in vr_clip; the
 * builder takes NULL for "no clip set".
 */
#include "../oracle/vr_oracle.c"

/* steps 1-3 of the clip contract (tests/clip_ref.c clip_segment) */
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

/* the transmittance byte of node (i, j, k): steps 1-5 */
static uint8_t shadow_node(const scene *s, const float *light, uint32_t S, float step, float cutoff, const float *clip, uint32_t max_steps,
                           uint32_t i, uint32_t j, uint32_t k) {
	const float scale = 2.0f / (float) (S - 1);
	const f3 n = f3_make(fmaf((float) i, scale, -1.0f), fmaf((float) j, scale, -1.0f), fmaf((float) k, scale, -1.0f));
	const f3 d = f3_sub(f3_make(light[0], light[1], light[2]), n);
	const float len2 = fmaf(d.z, d.z, fmaf(d.y, d.y, d.x * d.x));
	float T = 1.0f;
	if (len2 > 0) {
		const float il = rsqrt_nr(len2);
		const f3 u = f3_make(d.x * il, d.y * il, d.z * il);
		const float dist = len2 * il;
		float kx, ky;
		int hit = intersect(s, n, u, &kx, &ky);
		if (hit && clip != NULL) hit = clip_segment(clip, n, u, &kx, &ky);
		if (hit) {
			const float t_end = flmin(ky, dist);
			const f3 half = f3_make(0.5f * (float) s->dx, 0.5f * (float) s->dy, 0.5f * (float) s->dz);
			const f3 A = f3_make(u.x * half.x, u.y * half.y, u.z * half.z);
			const f3 B = f3_make(fmaf(n.x, half.x, half.x - 0.5f), fmaf(n.y, half.y, half.y - 0.5f), fmaf(n.z, half.z, half.z - 0.5f));
			float t = flmax(kx, 0) + step;
			uint32_t steps = 0;
			while (t <= t_end && steps < max_steps) {
				const float raw = sample_trilinear_raw(s, fmaf(t, A.x, B.x), fmaf(t, A.y, B.y), fmaf(t, A.z, B.z));
				const float a = tf_linear(s, raw).w;
				T = T * (1.0f - a);
				if (T < cutoff) { T = 0; break; }
				t += step;
				steps++;
			}
		}
	}
	const float scaled = T * 255.0f;
	return (uint8_t) (scaled + 0.5f);
}

/* q[S^3], x fastest; sampling VR_SAMPLE_TRILINEAR or _Q8; clip NULL = none set */
int shadow_build(const float *light, uint32_t S, float step, float cutoff, uint32_t sampling, const void *voxels, const uint32_t dims[3], uint32_t bpv,
                 const float *tf, const float *clip, uint8_t *q) {
	if (S < 2 || S > 256 || !(step >= 1.0f / 4096.0f) || (sampling != VR_SAMPLE_TRILINEAR && sampling != VR_SAMPLE_TRILINEAR_Q8))
		return 1;
	vr_params p;
	memset(&p, 0, sizeof p);
	p.sampling = sampling;
	const scene s = scene_of(&p, voxels, dims, bpv, tf, NULL);
	const uint32_t max_steps = (uint32_t) ceil(2.0 * sqrt(3.0) / (double) step) + 2u;
	#pragma omp parallel for schedule(dynamic, 4) collapse(2)
	for (uint32_t k = 0; k < S; k++)
		for (uint32_t j = 0; j < S; j++)
			for (uint32_t i = 0; i < S; i++)
				q[((size_t) k * S + j) * S + i] = shadow_node(&s, light, S, step, cutoff, clip, max_steps, i, j, k);
	return 0;
}

/* Tq at the model-space point pt, and the factor */
static float shadow_factor(const uint8_t *q, uint32_t S, float strength, f3 pt) {
	const float hs = 0.5f * (float) (S - 1), top = (float) (S - 1);
	const float c[3] = { pt.x, pt.y, pt.z };
	uint32_t idx[3];
	float w[3];
	for (int ax = 0; ax < 3; ax++) {
		float v = fmaf(c[ax], hs, hs);
		v = v < 0.0f ? 0.0f : (v > top ? top : v);                  /* fmed3(v, 0, S - 1) for the finite v of a frame */
		uint32_t i = (uint32_t) v;
		if (i > S - 2) i = S - 2;
		idx[ax] = i; w[ax] = v - (float) i;
	}
	const uint8_t *b = q + ((size_t) idx[2] * S + idx[1]) * S + idx[0];
	const size_t row = S, slab = (size_t) S * S;
	const float c00 = lerp((float) b[0], (float) b[1], w[0]), c10 = lerp((float) b[row], (float) b[row + 1], w[0]);
	const float c01 = lerp((float) b[slab], (float) b[slab + 1], w[0]), c11 = lerp((float) b[slab + row], (float) b[slab + row + 1], w[0]);
	const float tq = lerp(lerp(c00, c10, w[1]), lerp(c01, c11, w[1]), w[2]);
	return fmaf(strength * (1.0f / 255.0f), tq, 1.0f - strength);
}

/* clip_render_ray of tests/clip_ref.c for the TRILINEAR modes, with the scaling of dense samples; q NULL = no shadow */
static void shadow_render_ray(const scene *s, const float *clip, const uint8_t *q, uint32_t S, float strength, int px, int py, uint8_t *out_px) {
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
	while (kx <= ky) {
		const float xb = fmaf(kx, A.x, B.x), yb = fmaf(kx, A.y, B.y), zb = fmaf(kx, A.z, B.z);
		const float raw = sample_trilinear_raw(s, xb, yb, zb);
		f4 cur = tf_linear(s, raw);
		if (cur.w > 0.05f && p->light_kd > 0.01f) {
			const f3 d = f3_sub(light_pos, pt);
			const float inv = rsqrt_nr(fmaf(d.z, d.z, fmaf(d.y, d.y, d.x * d.x)));
			const f3 light_dir = f3_scale(d, inv);
			const float raw_l = sample_trilinear_raw(s, fmaf(light_dir.x, 0.01f * half.x, xb), fmaf(light_dir.y, 0.01f * half.y, yb),
			                                         fmaf(light_dir.z, 0.01f * half.z, zb));
			const float diffuse = (raw_l - raw) * (p->light_kd * (s->bpv == 1 ? (1.0f / 255.0f) : (1.0f / 65535.0f)));
			cur.x += diffuse; cur.y += diffuse; cur.z += diffuse;
		}
		if (q != NULL && cur.w > 0.05f) {                            /* the one addition: after the diffuse term, before the accumulation */
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

int shadow_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl,
                  const float *clip, const uint8_t *q, uint32_t S, float strength, uint8_t *out) {
	if (p->sampling != VR_SAMPLE_TRILINEAR && p->sampling != VR_SAMPLE_TRILINEAR_Q8)
		return 1;
	const scene s = scene_of(p, voxels, dims, bpv, tf, esl);
	memset(out, 0, (size_t) p->out_width * p->out_rows * 4);
	#pragma omp parallel for schedule(dynamic, 4)
	for (uint32_t y = 0; y < p->out_rows; y++)
		for (uint32_t x = 0; x < p->out_width; x++)
			shadow_render_ray(&s, clip, q, S, strength, (int) x, (int) y, out + ((size_t) y * p->out_width + x) * 4);
	return 0;
}
