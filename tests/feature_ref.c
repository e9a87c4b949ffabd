/*
 * feature_ref.c — every render feature of include/vr_hip.h restated with the CPU oracle's own statics, in one translation unit: the
 * maximum-intensity projection (vr_hip_render_mip), the shaded isosurface with depth (vr_hip_render_iso), the clip region
 * (vr_hip_set_clip), the light-source shadows (vr_hip_set_shadow), the gradient lighting (vr_hip_set_lighting), the pre-integrated
 * classification (vr_hip_set_preintegration) and the backdrop and hybrid frames (vr_hip_render_backdrop, vr_hip_render_hybrid).
 * TEST INFRASTRUCTURE: compiled once per session by tests/ref_library.py with the flags oracle/Makefile uses for libvr_oracle.so;
 * -ffp-contract=off is what makes a step stated once here the same arithmetic wherever it is inlined.
 *
 * It includes oracle/vr_oracle.c read-only, once.  There are two composite rays, on purpose:
 *   clip_render_ray      render_ray of oracle/vr_oracle.c (NEAREST and the TRILINEAR modes) with the segment clipped and nothing else.
 *                        tests/test_clip_model.py ties it to vro_render; it is the independent text the feature ray is held to.
 *   feature_render_ray   the TRILINEAR composite with every feature behind a switch of `features`; with all of them off it is
 *                        clip_render_ray, which the *_model.py tests hold it to byte for byte.
 * shadow_render, light_render, slab_render, backdrop_render and hybrid_render are wrappers of the feature ray: a tie between two of them
 * compares one text with itself.  tests/test_restatement_pins.py holds every entry point to the bytes of the separate texts this file
 * replaced.  One isosurface frame (iso_render, clip_iso_render, hybrid_render) and one MIP frame (mip_render, clip_mip_render).
 *
 * Whole frames only (pixel (x, y) of the view -> element y * out_width + x of the output and of both layers).
 * clip: box_min[3], box_max[3], plane[4] as in vr_clip.  lighting: ambient, diffuse, specular; shin: shininess_log2; NULL = the reference's
 * cue (light_kd).  q NULL = no shadow.
 */
#include "../oracle/vr_oracle.c"

#define SLAB_TF_MAX ((float) (VR_TF_SIZE - 1))

static int trilinear_mode(const vr_params *p) {
	return p->sampling == VR_SAMPLE_TRILINEAR || p->sampling == VR_SAMPLE_TRILINEAR_Q8;
}

static scene scene_of(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl) {
	scene s;
	s.p = p; s.vox8 = (const uint8_t *) voxels; s.vox16 = (const uint16_t *) voxels;
	s.dx = dims[0]; s.dy = dims[1]; s.dz = dims[2]; s.bpv = bpv;
	s.tf = (const f4 *) tf; s.esl = esl; s.min_bound = f3_make(-1, -1, -1); s.line_bits = NULL;
	return s;
}

/* ---- the clip region: steps 1-3 of the contract; returns the hit test on the narrowed segment ---- */
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

/* ---- shading ---- */
/* the central differences of the interpolated field one texel apart, at the texel coordinate (xb, yb, zb) */
static f3 field_gradient(const scene *s, float xb, float yb, float zb, f3 half) {
	const float gx = (sample_trilinear_raw(s, xb + 1.0f, yb, zb) - sample_trilinear_raw(s, xb - 1.0f, yb, zb)) * half.x;
	const float gy = (sample_trilinear_raw(s, xb, yb + 1.0f, zb) - sample_trilinear_raw(s, xb, yb - 1.0f, zb)) * half.y;
	const float gz = (sample_trilinear_raw(s, xb, yb, zb + 1.0f) - sample_trilinear_raw(s, xb, yb, zb - 1.0f)) * half.z;
	return f3_make(gx, gy, gz);
}

/* the reference's cue of a dense sample: the field a hundredth towards the light against the field here, scaled by light_kd */
static void shade_cue(const scene *s, f3 light_pos, f3 pt, float xb, float yb, float zb, f3 half, float raw, f4 *cur) {
	const f3 d = f3_sub(light_pos, pt);
	const float inv = rsqrt_nr(fmaf(d.z, d.z, fmaf(d.y, d.y, d.x * d.x)));
	const f3 light_dir = f3_scale(d, inv);
	const float raw_l = sample_trilinear_raw(s, fmaf(light_dir.x, 0.01f * half.x, xb), fmaf(light_dir.y, 0.01f * half.y, yb),
	                                         fmaf(light_dir.z, 0.01f * half.z, zb));
	const float diffuse = (raw_l - raw) * (s->p->light_kd * (s->bpv == 1 ? (1.0f / 255.0f) : (1.0f / 65535.0f)));
	cur->x += diffuse; cur->y += diffuse; cur->z += diffuse;
}

/* steps 1-4 of the lighting contract on a dense sample; returns 0 where the gradient is zero: the colour stays what it is */
static int shade_blinn_phong(const scene *s, const float *lighting, uint32_t shin, f3 light_pos, f3 direction, f3 pt, float xb, float yb, float zb,
                             f3 half, f4 *cur) {
	const float ka = lighting[0], kd = lighting[1], ks = lighting[2];
	/* 1. the isosurface's gradient */
	const f3 g = field_gradient(s, xb, yb, zb, half);
	const float gg = fmaf(g.z, g.z, fmaf(g.y, g.y, g.x * g.x));
	if (!(gg > 0.0f))
		return 0;
	/* 2. light */
	const float ig = rsqrt_nr(gg);
	const f3 dl = f3_sub(light_pos, pt);
	const float ll = fmaf(dl.z, dl.z, fmaf(dl.y, dl.y, dl.x * dl.x));
	float sd = 0.0f, sp = 0.0f;
	if (ll > 0.0f) {
		const float il = rsqrt_nr(ll);
		const float dot = fmaf(g.z, dl.z, fmaf(g.y, dl.y, g.x * dl.x));
		sd = fminf(fabsf((dot * ig) * il), 1.0f);
		/* 3. highlight */
		const float iv = rsqrt_nr(fmaf(direction.z, direction.z, fmaf(direction.y, direction.y, direction.x * direction.x)));
		const f3 h = f3_make(fmaf(-direction.x, iv, dl.x * il), fmaf(-direction.y, iv, dl.y * il), fmaf(-direction.z, iv, dl.z * il));
		const float hh = fmaf(h.z, h.z, fmaf(h.y, h.y, h.x * h.x));
		if (hh > 0.0f) {
			sp = fminf(fabsf((fmaf(g.z, h.z, fmaf(g.y, h.y, g.x * h.x)) * ig) * rsqrt_nr(hh)), 1.0f);
			for (uint32_t r = 0; r < shin; r++)
				sp = sp * sp;
		}
	}
	/* 4. colour; cur->w is untouched */
	const float m = fmaf(kd, sd, ka);
	const float spec = (ks * sp) * cur->w;
	cur->x = fmaf(cur->x, m, spec); cur->y = fmaf(cur->y, m, spec); cur->z = fmaf(cur->z, m, spec);
	return 1;
}

/* ---- the light grid ---- */
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

/* ---- the slab classification ---- */
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

/* What the slab modes of a frame need of its transfer function: the integral table in both precisions, and for mode 3 the leading
 * all-zero entries (zero_below) and the bound on a skippable raw value (skip_below), as the library forms them */
typedef struct {
	float K[4 * VR_TF_SIZE];
	double Kd[4 * VR_TF_SIZE];
	float skip_below, zero_below;
} slab_tables;

static void slab_tables_of(const float *tf, uint32_t bpv, slab_tables *t) {
	slab_build_integral(tf, t->K);
	slab_build_integral_double(tf, t->Kd);
	int zero = -1;
	while (zero + 1 < VR_TF_SIZE && tf[4 * (zero + 1)] == 0.0f && tf[4 * (zero + 1) + 1] == 0.0f && tf[4 * (zero + 1) + 2] == 0.0f && tf[4 * (zero + 1) + 3] == 0.0f)
		zero++;
	const float tf_scale = bpv == 1 ? (float) VR_TF_SIZE / 255.0f : (float) VR_TF_SIZE / 65535.0f;
	uint32_t below = 0;
	for (uint32_t P = 1; P <= (bpv == 1 ? 256u : 65536u); P <<= 1)
		if (zero >= 0 && fmaf((float) P, tf_scale, -0.5f) <= (float) zero) below = P;
	t->skip_below = (float) below; t->zero_below = (float) zero;
}

/* ---- the two composite rays ---- */
/* What a composite frame renders with.
 * mode: 0 = point classification, 1 = slab classification, 2 = slab classification with the wide-slab branch in double precision (K, K(t),
 * the difference and the division; rounded to fp32 once) — what the fp32 branch is held against; 3 = a wrong reading for the sensitivity
 * tests: a sample that the library may skip without resolving it — its value below the largest power of two P whose coordinate lies within
 * the transfer function's leading zeros, behind a predecessor within them too — counts as no predecessor at all for the next sample
 * (tp = tb), instead of handing its coordinate on.  Per ray: what a wave of the library skips is a subset of it.
 * layer_px / layer_depth: the pixel's elements of the opaque layer, NULL = no backdrop.
 * perturb: 0 = the contract.  The sensitivity test's three wrong readings of it: 1 = a sample at k == d is not composited (`k < d`);
 * 2 = the layer is not blended in once early termination has struck; 3 = bf = byte / 255. */
typedef struct {
	const float *clip;
	const float *lighting;
	uint32_t shin;
	const uint8_t *q;
	uint32_t S;
	float strength;
	uint32_t mode;
	const slab_tables *slab;
	const uint8_t *layer_px;
	float layer_depth;
	uint32_t perturb;
} features;

/* what the rays of a frame count: samples of the accumulation loop, those that took the wide-slab branch, those that took the narrow one,
 * dense samples (c.w > 0.05f) that were composited, and those among them that a lighting found with !(gg > 0) */
enum { N_SAMPLES, N_WIDE, N_NARROW, N_DENSE, N_FLAT, N_COUNTERS };

static void write_pixel(f4 acc, uint8_t *out_px) {
	out_px[0] = (uint8_t) map_float_int(acc.x, 256);
	out_px[1] = (uint8_t) map_float_int(acc.y, 256);
	out_px[2] = (uint8_t) map_float_int(acc.z, 256);
	out_px[3] = (uint8_t) map_float_int(acc.w, 256);
}

/* render_ray of oracle/vr_oracle.c (NEAREST and the TRILINEAR modes), the segment clipped: of `f` it reads the clip alone */
static void clip_render_ray(const scene *s, const features *f, int px, int py, uint8_t *out_px, uint64_t *n) {
	const vr_params *p = s->p;
	f3 origin, direction;
	float kx, ky;
	(void) n;
	get_ray(&p->view, px, py, &origin, &direction);
	if (!intersect(s, origin, direction, &kx, &ky))
		return;
	if (!clip_segment(f->clip, origin, direction, &kx, &ky))
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
	write_pixel(acc, out_px);
}

/* the leaping in front of the accumulation loop (TRILINEAR modes): kx and pt become those of the loop's first sample; 0 = there is none */
static int first_sample(const scene *s, f3 origin, f3 direction, float *kx, float ky, f3 *pt) {
	*pt = march_point(1, origin, direction, *kx);
	while (*kx <= ky) {
		if (s->p->esl && sample_data_esl(s, *pt))
			leap_empty_space(s, *pt, direction, kx);
		else
			break;
		*kx += s->p->ray_step;
		*pt = march_point(1, origin, direction, *kx);
	}
	return *kx <= ky;
}

/* The colour of the slab between the previous sample's transfer-function coordinate *tp and this one's (modes 1-3) */
static f4 slab_colour(const scene *s, const features *f, float raw, int *first, int *skipped, float *tp, uint64_t *n) {
	const float tf_scale = s->bpv == 1 ? (float) VR_TF_SIZE / 255.0f : (float) VR_TF_SIZE / 65535.0f;
	const float *tf = (const float *) s->tf;
	f4 cur;
	float tb = fmaf(raw, tf_scale, -0.5f);
	tb = tb < 0.0f ? 0.0f : (tb > SLAB_TF_MAX ? SLAB_TF_MAX : tb);          /* fmed3(.., 0, 127) for the finite coordinate of a frame */
	if (*first) *tp = tb;                                                   /* the loop's first sample */
	*first = 0;
	if (f->mode == 3) {                                                     /* the wrong reading: a skipped predecessor is none */
		if (*skipped) *tp = tb;
		*skipped = raw < f->slab->skip_below && *tp <= f->slab->zero_below;
	}
	const float d = tb - *tp;
	if (!(fabsf(d) >= 0.5f)) {                                              /* narrow slab: the lookup at its middle */
		n[N_NARROW]++;
		cur = slab_lookup(s, 0.5f * (*tp + tb));
	} else if (f->mode == 2) {
		n[N_WIDE]++;
		double kb[4], kp[4];
		slab_integral_at_double(tf, f->slab->Kd, tb, kb);
		slab_integral_at_double(tf, f->slab->Kd, *tp, kp);
		const double dd = (double) tb - (double) *tp;
		cur.x = (float) ((kb[0] - kp[0]) / dd); cur.y = (float) ((kb[1] - kp[1]) / dd);
		cur.z = (float) ((kb[2] - kp[2]) / dd); cur.w = (float) ((kb[3] - kp[3]) / dd);
	} else {                                                                /* wide slab: the mean of the transfer function over it */
		n[N_WIDE]++;
		const float r = 1.0f / d;
		const f4 kb = slab_integral_at(tf, f->slab->K, tb), kp = slab_integral_at(tf, f->slab->K, *tp);
		cur.x = (kb.x - kp.x) * r; cur.y = (kb.y - kp.y) * r; cur.z = (kb.z - kp.z) * r; cur.w = (kb.w - kp.w) * r;
	}
	*tp = tb;
	return cur;
}

/* The TRILINEAR composite with every feature: clip_render_ray with the looked-up colour replaced (mode), the cue replaced by steps 1-4
 * (a lighting; light_kd is then ignored), the shadow's factor on dense samples behind either, and the backdrop's three changes — the
 * narrowing of ky behind clip_segment, the hit test, the pixel */
static void feature_render_ray(const scene *s, const features *f, int px, int py, uint8_t *out_px, uint64_t *n) {
	const vr_params *p = s->p;
	const float d = f->layer_depth;
	const int surface = f->layer_px != NULL && d >= 0.0f;             /* an ordered compare: NaN and negative values mean no surface */
	f3 origin, direction, pt;
	float kx, ky;
	int hit;
	get_ray(&p->view, px, py, &origin, &direction);
	hit = intersect(s, origin, direction, &kx, &ky);
	if (hit)
		hit = clip_segment(f->clip, origin, direction, &kx, &ky);
	if (hit && surface) {
		ky = flmin(ky, d);
		hit = (kx < ky) && (ky > 0);
	}
	if (!hit || !first_sample(s, origin, direction, &kx, ky, &pt)) {
		if (surface) memcpy(out_px, f->layer_px, 4);
		return;
	}
	f4 acc = { 0, 0, 0, 0 };
	const f3 half = f3_make(0.5f * (float) s->dx, 0.5f * (float) s->dy, 0.5f * (float) s->dz);
	const f3 A = f3_make(direction.x * half.x, direction.y * half.y, direction.z * half.z);
	const f3 B = f3_make(fmaf(origin.x, half.x, half.x - 0.5f), fmaf(origin.y, half.y, half.y - 0.5f), fmaf(origin.z, half.z, half.z - 0.5f));
	const f3 light_pos = f3_make(p->view.light_pos[0], p->view.light_pos[1], p->view.light_pos[2]);
	int first = 1, skipped = 0, terminated = 0;
	float tp = 0.0f;
	while (kx <= ky) {
		if (f->perturb == 1 && surface && !(kx < d))
			break;
		const float xb = fmaf(kx, A.x, B.x), yb = fmaf(kx, A.y, B.y), zb = fmaf(kx, A.z, B.z);
		const float raw = sample_trilinear_raw(s, xb, yb, zb);
		n[N_SAMPLES]++;
		f4 cur = f->mode == 0 ? tf_linear(s, raw) : slab_colour(s, f, raw, &first, &skipped, &tp, n);
		if (cur.w > 0.05f) {
			n[N_DENSE]++;
			if (f->lighting != NULL)
				n[N_FLAT] += !shade_blinn_phong(s, f->lighting, f->shin, light_pos, direction, pt, xb, yb, zb, half, &cur);
			else if (p->light_kd > 0.01f)
				shade_cue(s, light_pos, pt, xb, yb, zb, half, raw, &cur);
			if (f->q != NULL) {                                          /* the shadow's factor, after the cue or step 4 */
				const float sf = shadow_factor(f->q, f->S, f->strength, pt);
				cur.x *= sf; cur.y *= sf; cur.z *= sf;
			}
		}
		const float t = 1 - acc.w;
		acc.x = fmaf(cur.x, t, acc.x); acc.y = fmaf(cur.y, t, acc.y);
		acc.z = fmaf(cur.z, t, acc.z); acc.w = fmaf(cur.w, t, acc.w);
		if (acc.w > p->ray_threshold) {
			terminated = 1;
			break;
		}
		kx += p->ray_step;
		pt = march_point(1, origin, direction, kx);
	}
	if (surface && !(f->perturb == 2 && terminated)) {
		const float t = 1.0f - acc.w;
		float bf[4];
		for (int ch = 0; ch < 4; ch++)
			bf[ch] = f->perturb == 3 ? (float) f->layer_px[ch] / 255.0f : ((float) f->layer_px[ch] + 0.5f) * (1.0f / 256.0f);
		acc.x = fmaf(bf[0], t, acc.x); acc.y = fmaf(bf[1], t, acc.y);
		acc.z = fmaf(bf[2], t, acc.z); acc.w = fmaf(bf[3], t, acc.w);
	}
	write_pixel(acc, out_px);
}

/* ---- the composite frame ---- */
typedef void ray_fn(const scene *s, const features *f, int px, int py, uint8_t *out_px, uint64_t *n);

/* Every pixel of the frame by `ray`; a pixel the ray does not write is zero.  layer_rgba / layer_depth: both NULL, or the backdrop; a pixel
 * reads its own layer elements before it writes, so `out` may be layer_rgba.  n_out: N_COUNTERS sums over the frame. */
static void composite_frame(const scene *s, const features *frame, ray_fn *ray, const uint8_t *layer_rgba, const float *layer_depth, uint8_t *out,
                            uint64_t *n_out) {
	const vr_params *p = s->p;
	uint64_t samples = 0, wide = 0, narrow = 0, dense = 0, flat = 0;
	#pragma omp parallel for schedule(dynamic, 4) reduction(+:samples, wide, narrow, dense, flat)
	for (uint32_t y = 0; y < p->out_rows; y++)
		for (uint32_t x = 0; x < p->out_width; x++) {
			const size_t px = (size_t) y * p->out_width + x;
			uint8_t b[4] = { 0, 0, 0, 0 }, o[4] = { 0, 0, 0, 0 };
			uint64_t n[N_COUNTERS] = { 0 };
			features f = *frame;
			if (layer_rgba != NULL) {
				memcpy(b, layer_rgba + 4 * px, 4);
				f.layer_px = b; f.layer_depth = layer_depth[px];
			}
			ray(s, &f, (int) x, (int) y, o, n);
			memcpy(out + 4 * px, o, 4);
			samples += n[N_SAMPLES]; wide += n[N_WIDE]; narrow += n[N_NARROW]; dense += n[N_DENSE]; flat += n[N_FLAT];
		}
	n_out[N_SAMPLES] = samples; n_out[N_WIDE] = wide; n_out[N_NARROW] = narrow; n_out[N_DENSE] = dense; n_out[N_FLAT] = flat;
}

/* the frame of the feature ray under the arguments the entry points share; n_out as above */
static int feature_frame(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl,
                         const float *clip, const float *lighting, uint32_t shin, const uint8_t *q, uint32_t S, float strength, uint32_t mode,
                         uint32_t perturb, const uint8_t *layer_rgba, const float *layer_depth, uint8_t *out, uint64_t *n_out) {
	if (!trilinear_mode(p))
		return 1;
	const scene s = scene_of(p, voxels, dims, bpv, tf, esl);
	slab_tables tables;
	slab_tables_of(tf, bpv, &tables);
	const features f = { clip, lighting, shin, q, S, strength, mode, &tables, NULL, -1.0f, perturb };
	composite_frame(&s, &f, feature_render_ray, layer_rgba, layer_depth, out, n_out);
	return 0;
}

int clip_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl,
                const float *clip, uint8_t *out) {
	const scene s = scene_of(p, voxels, dims, bpv, tf, esl);
	const features f = { .clip = clip };
	uint64_t n[N_COUNTERS];
	composite_frame(&s, &f, clip_render_ray, NULL, NULL, out, n);
	return 0;
}

int shadow_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl,
                  const float *clip, const uint8_t *q, uint32_t S, float strength, uint8_t *out) {
	uint64_t n[N_COUNTERS];
	return feature_frame(p, voxels, dims, bpv, tf, esl, clip, NULL, 0, q, S, strength, 0, 0, NULL, NULL, out, n);
}

/* counters_out[2]: dense samples (c.w > 0.05f) that were composited, and those among them with !(gg > 0) */
int light_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl,
                 const float *clip, const float *lighting, uint32_t shin, const uint8_t *q, uint32_t S, float strength, uint8_t *out,
                 uint64_t *counters_out) {
	uint64_t n[N_COUNTERS];
	if (feature_frame(p, voxels, dims, bpv, tf, esl, clip, lighting, shin, q, S, strength, 0, 0, NULL, NULL, out, n))
		return 1;
	counters_out[0] = n[N_DENSE]; counters_out[1] = n[N_FLAT];
	return 0;
}

/* mode 0-3 as `features` has them.  counters_out[3]: samples of the accumulation loop, those that took the wide-slab branch, those that
 * took the narrow one */
int slab_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl,
                const float *clip, const float *lighting, uint32_t shin, const uint8_t *q, uint32_t S, float strength, uint32_t mode,
                uint8_t *out, uint64_t *counters_out) {
	uint64_t n[N_COUNTERS];
	if (mode > 3 || feature_frame(p, voxels, dims, bpv, tf, esl, clip, lighting, shin, q, S, strength, mode, 0, NULL, NULL, out, n))
		return 1;
	counters_out[0] = n[N_SAMPLES]; counters_out[1] = n[N_WIDE]; counters_out[2] = n[N_NARROW];
	return 0;
}

/* layer_rgba / layer_depth: out_width * out_rows RGBA8 words / floats, or both NULL: the bytes of slab_render.  `out` may be layer_rgba.
 * mode 0 or 1 */
int backdrop_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl,
                    const float *clip, const float *lighting, uint32_t shin, const uint8_t *q, uint32_t S, float strength, uint32_t mode,
                    uint32_t perturb, const uint8_t *layer_rgba, const float *layer_depth, uint8_t *out) {
	uint64_t n[N_COUNTERS];
	if (mode > 1 || perturb > 3 || (layer_rgba == NULL) != (layer_depth == NULL))
		return 1;
	return feature_frame(p, voxels, dims, bpv, tf, esl, clip, lighting, shin, q, S, strength, mode, perturb, layer_rgba, layer_depth, out, n);
}

/* What the layer generator of tests/backdrop_helpers.py places its depths by: per pixel { kx, ky, k0 } — the clipped segment and the k of the
 * first sample of the accumulation loop of the frame WITHOUT a backdrop (behind the leaping; NaN where the ray is fully empty) —, or three
 * NaNs for a miss.  Samples of that frame lie at k0, k0 + step, (k0 + step) + step, ... */
int backdrop_segments(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl,
                      const float *clip, float *seg_out) {
	const scene s = scene_of(p, voxels, dims, bpv, tf, esl);
	#pragma omp parallel for schedule(dynamic, 4)
	for (uint32_t y = 0; y < p->out_rows; y++)
		for (uint32_t x = 0; x < p->out_width; x++) {
			float *o = seg_out + 3 * ((size_t) y * p->out_width + x);
			f3 origin, direction, pt;
			float kx, ky;
			o[0] = o[1] = o[2] = NAN;
			get_ray(&p->view, (int) x, (int) y, &origin, &direction);
			if (!intersect(&s, origin, direction, &kx, &ky) || !clip_segment(clip, origin, direction, &kx, &ky))
				continue;
			o[0] = kx; o[1] = ky;
			if (first_sample(&s, origin, direction, &kx, ky, &pt)) o[2] = kx;
		}
	return 0;
}

/* ---- the maximum-intensity projection ---- */
/* The ray is get_ray + intersect, the sample sequence is the oracle's march with leaping off (k accumulated by repeated addition, the
 * position formed from k), a sample is sample_nearest at march_point or sample_trilinear_raw at fma(k, A, B), the colour is
 * transfer_fn[s8 / TF_RATIO] or tf_linear, the pixel is map_float_int of the colour: no arithmetic of its own.  clip NULL = none;
 * raw_out (may be NULL) receives the per-pixel maximum — the integer for NEAREST, the bits of the float for TRILINEAR — and 0xffffffff
 * for rays without a segment. */
static void mip_frame(const scene *s, const float *clip, uint8_t *out, uint32_t *raw_out) {
	const vr_params *p = s->p;
	memset(out, 0, (size_t) p->out_width * p->out_rows * 4);
	#pragma omp parallel for schedule(dynamic, 4)
	for (uint32_t y = 0; y < p->out_rows; y++)
		for (uint32_t x = 0; x < p->out_width; x++) {
			f3 o, d;
			float kx, ky;
			const size_t px = (size_t) y * p->out_width + x;
			if (raw_out != NULL) raw_out[px] = 0xffffffffu;
			get_ray(&p->view, (int) x, (int) y, &o, &d);
			if (!intersect(s, o, d, &kx, &ky))
				continue;
			if (clip != NULL && !clip_segment(clip, o, d, &kx, &ky))
				continue;
			const int fused = p->sampling != VR_SAMPLE_NEAREST;
			const f3 half = f3_make(0.5f * (float) s->dx, 0.5f * (float) s->dy, 0.5f * (float) s->dz);
			const f3 A = f3_make(d.x * half.x, d.y * half.y, d.z * half.z);
			const f3 B = f3_make(fmaf(o.x, half.x, half.x - 0.5f), fmaf(o.y, half.y, half.y - 0.5f), fmaf(o.z, half.z, half.z - 0.5f));
			uint32_t mi = 0;
			float mf = 0.0f;
			while (kx <= ky) {
				if (!fused) {
					const uint32_t v = sample_nearest(s, march_point(0, o, d, kx));
					if (v > mi) mi = v;
				} else {
					const float r = sample_trilinear_raw(s, fmaf(kx, A.x, B.x), fmaf(kx, A.y, B.y), fmaf(kx, A.z, B.z));
					if (r > mf) mf = r;
				}
				kx += p->ray_step;
			}
			f4 c;
			if (!fused) {
				const uint32_t s8 = s->bpv == 1 ? mi : mi >> 8;
				c = s->tf[s8 / VR_TF_RATIO];
				if (raw_out != NULL) raw_out[px] = mi;
			} else {
				c = tf_linear(s, mf);
				if (raw_out != NULL) memcpy(&raw_out[px], &mf, 4);
			}
			write_pixel(c, out + 4 * px);
		}
}

int mip_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, uint8_t *out, uint32_t *raw_out) {
	const scene s = scene_of(p, voxels, dims, bpv, tf, NULL);
	mip_frame(&s, NULL, out, raw_out);
	return 0;
}

int clip_mip_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const float *clip, uint8_t *out) {
	const scene s = scene_of(p, voxels, dims, bpv, tf, NULL);
	mip_frame(&s, clip, out, NULL);
	return 0;
}

/* ---- the shaded isosurface with depth ---- */
/* the 3x3x3-dilated block maxima of vro_volume_minmax's grid (tests/mip_bound_ref.c) */
void iso_dilated_maxima(const void *voxels, const uint32_t dims[3], uint32_t bpv, uint8_t *dil /* 32768 */, uint32_t *block_dims_out) {
	static uint8_t mm[65536];
	float bs[3];
	vro_volume_minmax(voxels, dims, bpv, mm, block_dims_out, bs);
	for (int z = 0; z < 32; z++) for (int y = 0; y < 32; y++) for (int x = 0; x < 32; x++) {
		uint32_t a = 0;
		for (int dz = -1; dz <= 1; dz++) for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
			int nx = x + dx, ny = y + dy, nz = z + dz;
			if (nx < 0 || ny < 0 || nz < 0 || nx > 31 || ny > 31 || nz > 31) continue;
			uint32_t v = mm[2 * ((nz * 32 + ny) * 32 + nx) + 1];
			if (v > a) a = v;
		}
		dil[(z * 32 + y) * 32 + x] = (uint8_t) a;
	}
}

/* The ray is get_ray + intersect (+ clip_segment; clip NULL = none), the sample sequence is the oracle's march with leaping off, a field
 * value is sample_trilinear_raw at fma(k, A, B), the base colour is tf_linear of the level, the light vector is normalised with rsqrt_nr at
 * march_point, the pixel is map_float_int of the shaded colour.  Its own arithmetic is the bisection (step 4 of the contract) and the
 * gradient shading (step 6), nothing else.  depth_out: k* or -1.  ray_out (may be NULL): origin and direction of every pixel's ray, six
 * floats.  counters_out[3]: samples of the march, fetches of the march, surface pixels.  dilated: NULL, or the 32^3 3x3x3-dilated block
 * maxima (high bytes for 2-byte voxels) and the block edge: the march then skips the fetch of every sample whose widened bound is below
 * the level, as the kernel may — a skipped sample counts as "below the level" without being looked at. */
static void iso_frame(const scene *s, float level, uint32_t refine, const float *clip, const uint8_t *dilated, uint32_t block_dims, uint8_t *out,
                      float *depth_out, float *ray_out, uint64_t *counters_out) {
	const vr_params *p = s->p;
	const int q8 = p->sampling == VR_SAMPLE_TRILINEAR_Q8;
	const f3 half = f3_make(0.5f * (float) s->dx, 0.5f * (float) s->dy, 0.5f * (float) s->dz);
	const f3 light_pos = f3_make(p->view.light_pos[0], p->view.light_pos[1], p->view.light_pos[2]);
	const f4 base = tf_linear(s, level);
	uint64_t samples = 0, fetches = 0, hits = 0;
	memset(out, 0, (size_t) p->out_width * p->out_rows * 4);
	#pragma omp parallel for schedule(dynamic, 4) reduction(+:samples, fetches, hits)
	for (uint32_t y = 0; y < p->out_rows; y++)
		for (uint32_t x = 0; x < p->out_width; x++) {
			f3 o, d;
			float kx, ky;
			const size_t px = (size_t) y * p->out_width + x;
			depth_out[px] = -1.0f;
			get_ray(&p->view, (int) x, (int) y, &o, &d);
			if (ray_out != NULL) { float *r = ray_out + 6 * px; r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z; }
			if (!intersect(s, o, d, &kx, &ky))
				continue;
			if (clip != NULL && !clip_segment(clip, o, d, &kx, &ky))
				continue;
			const f3 A = f3_make(d.x * half.x, d.y * half.y, d.z * half.z);
			const f3 B = f3_make(fmaf(o.x, half.x, half.x - 0.5f), fmaf(o.y, half.y, half.y - 0.5f), fmaf(o.z, half.z, half.z - 0.5f));
#define V_AT(k) sample_trilinear_raw(s, fmaf((k), A.x, B.x), fmaf((k), A.y, B.y), fmaf((k), A.z, B.z))
			/* steps 2, 3: the first sample at or above the level */
			int found = 0, first = 1;
			float lo = kx, hi = kx;
			while (kx <= ky) {
				int fetch = 1;
				samples++;
				if (dilated != NULL) {
					const f3 pos = march_point(1, o, d, kx);
					const uint32_t bx = map_float_int((pos.x + 1) * 0.5f, s->dx) / block_dims, by = map_float_int((pos.y + 1) * 0.5f, s->dy) / block_dims,
					               bz = map_float_int((pos.z + 1) * 0.5f, s->dz) / block_dims;
					const uint32_t hb = dilated[(bz * 32 + by) * 32 + bx];
					const float bound = s->bpv == 1 ? (float) hb : (q8 ? (float) ((hb + 1u) << 8) : (float) ((hb << 8) | 0xffu));
					fetch = !(bound < level);
				}
				if (fetch) {
					fetches++;
					if (V_AT(kx) >= level) { found = 1; hi = kx; if (first) lo = kx; break; }
				}
				lo = kx;
				first = 0;
				kx += p->ray_step;
			}
			if (!found)
				continue;
			hits++;
			/* step 4: bisection (a hit at the first sample has lo == hi and stays where it is) */
			if (!first)
				for (uint32_t r = 0; r < refine; r++) {
					const float mid = 0.5f * (lo + hi);
					if (V_AT(mid) >= level) hi = mid; else lo = mid;
				}
#undef V_AT
			depth_out[px] = hi;
			/* step 6: two-sided diffuse shading from central differences one texel apart */
			float f = 1.0f;
			if (!(p->light_kd <= 0.01f)) {
				const f3 g = field_gradient(s, fmaf(hi, A.x, B.x), fmaf(hi, A.y, B.y), fmaf(hi, A.z, B.z), half);
				const float gg = fmaf(g.z, g.z, fmaf(g.y, g.y, g.x * g.x));
				float sh = 0.0f;
				if (gg > 0.0f) {
					const f3 pt = march_point(1, o, d, hi);
					const f3 dl = f3_sub(light_pos, pt);
					const float il = rsqrt_nr(fmaf(dl.z, dl.z, fmaf(dl.y, dl.y, dl.x * dl.x)));
					const float dot = fmaf(g.z, dl.z, fmaf(g.y, dl.y, g.x * dl.x));
					sh = fminf(fabsf((dot * rsqrt_nr(gg)) * il), 1.0f);
				}
				f = fmaf(p->light_kd, sh, 1.0f - p->light_kd);
			}
			const f4 c = { base.x * f, base.y * f, base.z * f, base.w };
			write_pixel(c, out + 4 * px);
		}
	if (counters_out != NULL) { counters_out[0] = samples; counters_out[1] = fetches; counters_out[2] = hits; }
}

int iso_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, float level, uint32_t refine,
               const uint8_t *dilated, uint32_t block_dims, uint8_t *out, float *depth_out, uint64_t *counters_out) {
	if (!trilinear_mode(p))
		return 1;
	const scene s = scene_of(p, voxels, dims, bpv, tf, NULL);
	iso_frame(&s, level, refine, NULL, dilated, block_dims, out, depth_out, NULL, counters_out);
	return 0;
}

/* the isosurface with the segment clipped (without the skipping emulation: skipping never changes a frame) */
int clip_iso_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, float level, uint32_t refine,
                    const float *clip, uint8_t *out, float *depth_out, float *ray_out) {
	if (!trilinear_mode(p))
		return 1;
	const scene s = scene_of(p, voxels, dims, bpv, tf, NULL);
	iso_frame(&s, level, refine, clip, NULL, 0, out, depth_out, ray_out, NULL);
	return 0;
}

/* The hybrid: the clipped isosurface frame into iso_out (may be NULL) and depth_out, then backdrop_render over it into out.  The
 * isosurface sees the clip and light_kd and ignores the shadow, the lighting and the classification mode; the composite pass sees all. */
int hybrid_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl,
                  const float *clip, const float *lighting, uint32_t shin, const uint8_t *q, uint32_t S, float strength, uint32_t mode,
                  uint32_t perturb, float level, uint32_t refine, uint8_t *out, float *depth_out, uint8_t *iso_out) {
	if (clip_iso_render(p, voxels, dims, bpv, tf, level, refine, clip, out, depth_out, NULL))
		return 1;
	if (iso_out != NULL) memcpy(iso_out, out, (size_t) p->out_width * p->out_rows * 4);
	return backdrop_render(p, voxels, dims, bpv, tf, esl, clip, lighting, shin, q, S, strength, mode, perturb, out, depth_out, out);
}
