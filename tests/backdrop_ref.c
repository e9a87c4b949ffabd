/*
 * backdrop_ref.c — the backdrop and hybrid frames of include/vr_hip.h (vr_hip_render_backdrop, vr_hip_render_hybrid) restated with the CPU
 * oracle's own statics: the composite frame whose rays stop at the depth of an opaque RGBA8 layer and whose accumulated colour is blended
 * over the layer's, and the isosurface of the same volume as that layer.
 * TEST INFRASTRUCTURE: compiled on demand by tests/backdrop_helpers.py with the flags oracle/Makefile uses for libvr_oracle.so.
 *
 * It includes tests/slab_ref.c, and through it tests/light_ref.c, tests/shadow_ref.c and oracle/vr_oracle.c, read-only: clip_segment,
 * scene_of, shadow_factor, the integral table and the lookups are those restatements'.  backdrop_render_ray is slab_render_ray with the
 * three changes of the contract — the narrowing of ky behind clip_segment, the hit test, the pixel —; with NULL layers it is slab_render_ray
 * (modes 0 and 1), which tests/test_backdrop_model.py holds it to byte for byte.  The isosurface of the hybrid is tests/iso_ref.c's march
 * under the clip as tests/clip_ref.c has it (neither can be included next to slab_ref.c: all three bring the oracle's statics), restated
 * here as hybrid_iso_frame and held to clip_iso_render by the same test file.
 *
 * Whole frames only (pixel (x, y) of the view -> element y * out_width + x of the output and of both layers).  lighting NULL = the
 * reference's cue (light_kd); q NULL = no shadow.  mode: 0 = point classification, 1 = slab classification.
 * perturb: 0 = the contract.  The sensitivity test's three wrong readings of it: 1 = a sample at k == d is not composited (`k < d`);
 * 2 = the layer is not blended in once early termination has struck; 3 = bf = byte / 255.
 */
#include "slab_ref.c"

static void backdrop_render_ray(const scene *s, const float *K, const float *clip, const float *lighting, uint32_t shin, const uint8_t *q,
                                uint32_t S, float strength, uint32_t mode, uint32_t perturb, const uint8_t *layer_px, float d, int px, int py,
                                uint8_t *out_px) {
	const vr_params *p = s->p;
	const int surface = layer_px != NULL && d >= 0.0f;                 /* an ordered compare: NaN and negative values mean no surface */
	f3 origin, direction;
	float kx, ky;
	int hit;
	get_ray(&p->view, px, py, &origin, &direction);
	hit = intersect(s, origin, direction, &kx, &ky);
	if (hit)
		hit = clip_segment(clip, origin, direction, &kx, &ky);
	if (hit && surface) {
		ky = flmin(ky, d);
		hit = (kx < ky) && (ky > 0);
	}
	if (!hit) {
		if (surface) memcpy(out_px, layer_px, 4);
		return;
	}
	f3 pt = march_point(1, origin, direction, kx);
	while (kx <= ky) {
		if (p->esl && sample_data_esl(s, pt))
			leap_empty_space(s, pt, direction, &kx);
		else
			break;
		kx += p->ray_step;
		pt = march_point(1, origin, direction, kx);
	}
	if (kx > ky) {
		if (surface) memcpy(out_px, layer_px, 4);
		return;
	}
	f4 acc = { 0, 0, 0, 0 };
	const f3 half = f3_make(0.5f * (float) s->dx, 0.5f * (float) s->dy, 0.5f * (float) s->dz);
	const f3 A = f3_make(direction.x * half.x, direction.y * half.y, direction.z * half.z);
	const f3 B = f3_make(fmaf(origin.x, half.x, half.x - 0.5f), fmaf(origin.y, half.y, half.y - 0.5f), fmaf(origin.z, half.z, half.z - 0.5f));
	const f3 light_pos = f3_make(p->view.light_pos[0], p->view.light_pos[1], p->view.light_pos[2]);
	const float tf_scale = s->bpv == 1 ? (float) VR_TF_SIZE / 255.0f : (float) VR_TF_SIZE / 65535.0f;
	const float *tf = (const float *) s->tf;
	int first = 1, terminated = 0;
	float tp = 0.0f;
	while (kx <= ky) {
		if (perturb == 1 && surface && !(kx < d))
			break;
		const float xb = fmaf(kx, A.x, B.x), yb = fmaf(kx, A.y, B.y), zb = fmaf(kx, A.z, B.z);
		const float raw = sample_trilinear_raw(s, xb, yb, zb);
		f4 cur;
		if (mode == 0)
			cur = tf_linear(s, raw);
		else {
			float tb = fmaf(raw, tf_scale, -0.5f);
			tb = tb < 0.0f ? 0.0f : (tb > SLAB_TF_MAX ? SLAB_TF_MAX : tb);
			if (first) tp = tb;
			first = 0;
			const float dt = tb - tp;
			if (!(fabsf(dt) >= 0.5f))
				cur = slab_lookup(s, 0.5f * (tp + tb));
			else {
				const float r = 1.0f / dt;
				const f4 kb = slab_integral_at(tf, K, tb), kp = slab_integral_at(tf, K, tp);
				cur.x = (kb.x - kp.x) * r; cur.y = (kb.y - kp.y) * r; cur.z = (kb.z - kp.z) * r; cur.w = (kb.w - kp.w) * r;
			}
			tp = tb;
		}
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
			const f3 dd = f3_sub(light_pos, pt);
			const float inv = rsqrt_nr(fmaf(dd.z, dd.z, fmaf(dd.y, dd.y, dd.x * dd.x)));
			const f3 light_dir = f3_scale(dd, inv);
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
		if (acc.w > p->ray_threshold) {
			terminated = 1;
			break;
		}
		kx += p->ray_step;
		pt = march_point(1, origin, direction, kx);
	}
	if (surface && !(perturb == 2 && terminated)) {
		const float t = 1.0f - acc.w;
		float bf[4];
		for (int ch = 0; ch < 4; ch++)
			bf[ch] = perturb == 3 ? (float) layer_px[ch] / 255.0f : ((float) layer_px[ch] + 0.5f) * (1.0f / 256.0f);
		acc.x = fmaf(bf[0], t, acc.x); acc.y = fmaf(bf[1], t, acc.y);
		acc.z = fmaf(bf[2], t, acc.z); acc.w = fmaf(bf[3], t, acc.w);
	}
	out_px[0] = (uint8_t) map_float_int(acc.x, 256);
	out_px[1] = (uint8_t) map_float_int(acc.y, 256);
	out_px[2] = (uint8_t) map_float_int(acc.z, 256);
	out_px[3] = (uint8_t) map_float_int(acc.w, 256);
}

/* layer_rgba / layer_depth: out_width * out_rows RGBA8 words / floats, or both NULL: the bytes of slab_render.  `out` may be layer_rgba. */
int backdrop_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl,
                    const float *clip, const float *lighting, uint32_t shin, const uint8_t *q, uint32_t S, float strength, uint32_t mode,
                    uint32_t perturb, const uint8_t *layer_rgba, const float *layer_depth, uint8_t *out) {
	if ((p->sampling != VR_SAMPLE_TRILINEAR && p->sampling != VR_SAMPLE_TRILINEAR_Q8) || mode > 1 || perturb > 3 || (layer_rgba == NULL) != (layer_depth == NULL))
		return 1;
	const scene s = scene_of(p, voxels, dims, bpv, tf, esl);
	float K[4 * VR_TF_SIZE];
	slab_build_integral(tf, K);
	#pragma omp parallel for schedule(dynamic, 4)
	for (uint32_t y = 0; y < p->out_rows; y++)
		for (uint32_t x = 0; x < p->out_width; x++) {
			const size_t px = (size_t) y * p->out_width + x;
			uint8_t b[4] = { 0, 0, 0, 0 }, o[4] = { 0, 0, 0, 0 };
			if (layer_rgba != NULL) memcpy(b, layer_rgba + 4 * px, 4);           /* a pixel reads its own layer elements first */
			backdrop_render_ray(&s, K, clip, lighting, shin, q, S, strength, mode, perturb, layer_rgba != NULL ? b : NULL,
			                    layer_depth != NULL ? layer_depth[px] : -1.0f, (int) x, (int) y, o);
			memcpy(out + 4 * px, o, 4);
		}
	return 0;
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
			f3 origin, direction;
			float kx, ky;
			o[0] = o[1] = o[2] = NAN;
			get_ray(&p->view, (int) x, (int) y, &origin, &direction);
			if (!intersect(&s, origin, direction, &kx, &ky) || !clip_segment(clip, origin, direction, &kx, &ky))
				continue;
			o[0] = kx; o[1] = ky;
			f3 pt = march_point(1, origin, direction, kx);
			while (kx <= ky) {
				if (p->esl && sample_data_esl(&s, pt))
					leap_empty_space(&s, pt, direction, &kx);
				else
					break;
				kx += p->ray_step;
				pt = march_point(1, origin, direction, kx);
			}
			if (kx <= ky) o[2] = kx;
		}
	return 0;
}

/* iso_render of tests/iso_ref.c with the segment clipped, as clip_iso_render of tests/clip_ref.c has it */
static void hybrid_iso_frame(const vr_params *p, const scene *s, float level, uint32_t refine, const float *clip, uint8_t *out, float *depth_out) {
	const f3 half = f3_make(0.5f * (float) s->dx, 0.5f * (float) s->dy, 0.5f * (float) s->dz);
	const f3 light_pos = f3_make(p->view.light_pos[0], p->view.light_pos[1], p->view.light_pos[2]);
	const f4 base = tf_linear(s, level);
	memset(out, 0, (size_t) p->out_width * p->out_rows * 4);
	#pragma omp parallel for schedule(dynamic, 4)
	for (uint32_t y = 0; y < p->out_rows; y++)
		for (uint32_t x = 0; x < p->out_width; x++) {
			f3 o, d;
			float kx, ky;
			const size_t px = (size_t) y * p->out_width + x;
			depth_out[px] = -1.0f;
			get_ray(&p->view, (int) x, (int) y, &o, &d);
			if (!intersect(s, o, d, &kx, &ky))
				continue;
			if (!clip_segment(clip, o, d, &kx, &ky))
				continue;
			const f3 A = f3_make(d.x * half.x, d.y * half.y, d.z * half.z);
			const f3 B = f3_make(fmaf(o.x, half.x, half.x - 0.5f), fmaf(o.y, half.y, half.y - 0.5f), fmaf(o.z, half.z, half.z - 0.5f));
#define V_AT(k) sample_trilinear_raw(s, fmaf((k), A.x, B.x), fmaf((k), A.y, B.y), fmaf((k), A.z, B.z))
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
				const float gx = (sample_trilinear_raw(s, xb + 1.0f, yb, zb) - sample_trilinear_raw(s, xb - 1.0f, yb, zb)) * half.x;
				const float gy = (sample_trilinear_raw(s, xb, yb + 1.0f, zb) - sample_trilinear_raw(s, xb, yb - 1.0f, zb)) * half.y;
				const float gz = (sample_trilinear_raw(s, xb, yb, zb + 1.0f) - sample_trilinear_raw(s, xb, yb, zb - 1.0f)) * half.z;
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
}

/* The hybrid: the clipped isosurface frame into iso_out (may be NULL) and depth_out, then backdrop_render over it into out.  The
 * isosurface sees the clip and light_kd and ignores the shadow, the lighting and the classification mode; the composite pass sees all. */
int hybrid_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl,
                  const float *clip, const float *lighting, uint32_t shin, const uint8_t *q, uint32_t S, float strength, uint32_t mode,
                  uint32_t perturb, float level, uint32_t refine, uint8_t *out, float *depth_out, uint8_t *iso_out) {
	if (p->sampling != VR_SAMPLE_TRILINEAR && p->sampling != VR_SAMPLE_TRILINEAR_Q8)
		return 1;
	const scene s = scene_of(p, voxels, dims, bpv, tf, NULL);
	hybrid_iso_frame(p, &s, level, refine, clip, out, depth_out);
	if (iso_out != NULL) memcpy(iso_out, out, (size_t) p->out_width * p->out_rows * 4);
	return backdrop_render(p, voxels, dims, bpv, tf, esl, clip, lighting, shin, q, S, strength, mode, perturb, out, depth_out, out);
}
