/*
 * label_ref.c — the labelled composite frame of include/vr_hip.h (vr_hip_render_labelled) restated with the CPU oracle's own statics.
 * TEST INFRASTRUCTURE: compiled once per session by tests/label_helpers.py through ref_library.compile_test_library, with the flags of
 * tests/feature_ref.c.
 *
 * It includes tests/feature_ref.c read-only, once: the ray is get_ray + intersect + clip_segment, the leaping is first_sample, a sample is
 * sample_trilinear_raw at fma(k, A, B), its colour tf_linear, the shading shade_cue or shade_blinn_phong, the shadow shadow_factor, the
 * pixel write_pixel — the texts the composite restatements (clip_render, light_render, shadow_render) are made of.  Its own arithmetic is
 * steps 3 and 4 of the label contract (the nearest label and the table entry) and the loop that places them, nothing else.
 *
 * Whole frames only.  clip: the ten floats of vr_clip, never NULL (a labelled frame always runs the clip's arithmetic: the identity clip
 * when none is set).  lighting NULL = the reference's cue; q NULL = no shadow.  labels: one byte per voxel, x fastest, the volume's dims.
 * table: 256 entries of 5 floats { colour[3], mix, opacity }.
 * perturb: 0 = the contract.  The sensitivity test's wrong readings of it: 1 = the index without the + 0.5f (floor); 2 = the entry applied
 * behind the dense test and the shading; 3 = opacity scales alpha only; 4 = `mix` blends towards colour times the SCALED c.w.
 */
#include "feature_ref.c"

enum { LABEL_FLOOR = 1, LABEL_AFTER_SHADING = 2, LABEL_ALPHA_ONLY = 3, LABEL_MIX_SCALED = 4 };

static uint32_t label_axis(float x, uint32_t n, uint32_t perturb) {
	float v = perturb == LABEL_FLOOR ? x : x + 0.5f;
	const float top = (float) (n - 1);
	v = v < 0.0f ? 0.0f : (v > top ? top : v);                      /* fmed3(v, 0, N - 1) for the finite coordinate of a frame */
	return (uint32_t) v;
}

static void label_apply(const float *e, uint32_t perturb, f4 *c) {
	const float w = perturb == LABEL_MIX_SCALED ? c->w * e[4] : c->w;
	c->x = fmaf(e[3], fmaf(e[0], w, -c->x), c->x);
	c->y = fmaf(e[3], fmaf(e[1], w, -c->y), c->y);
	c->z = fmaf(e[3], fmaf(e[2], w, -c->z), c->z);
	if (perturb != LABEL_ALPHA_ONLY) { c->x = c->x * e[4]; c->y = c->y * e[4]; c->z = c->z * e[4]; }
	c->w = c->w * e[4];
}

/* out: the frame.  count_out (may be NULL): per pixel the samples of its accumulation loop.  label_count_out (may be NULL): 256 sums over the
 * frame — the samples of the accumulation loops whose looked-up alpha (before the entry) is above 0, by label. */
int label_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl, const float *clip,
                 const float *lighting, uint32_t shin, const uint8_t *q, uint32_t S, float strength, const uint8_t *labels, const float *table,
                 uint32_t perturb, uint8_t *out, uint32_t *count_out, uint64_t *label_count_out) {
	if (!trilinear_mode(p) || perturb > 4 || clip == NULL || labels == NULL || table == NULL)
		return 1;
	const scene s = scene_of(p, voxels, dims, bpv, tf, esl);
	uint64_t by_label[256] = { 0 };
	memset(out, 0, (size_t) p->out_width * p->out_rows * 4);
	#pragma omp parallel for schedule(dynamic, 4) reduction(+:by_label[:256])
	for (uint32_t y = 0; y < p->out_rows; y++)
		for (uint32_t x = 0; x < p->out_width; x++) {
			f3 o, d, pt;
			float kx, ky;
			const size_t px = (size_t) y * p->out_width + x;
			if (count_out != NULL) count_out[px] = 0;
			get_ray(&p->view, (int) x, (int) y, &o, &d);
			if (!intersect(&s, o, d, &kx, &ky) || !clip_segment(clip, o, d, &kx, &ky) || !first_sample(&s, o, d, &kx, ky, &pt))
				continue;
			f4 acc = { 0, 0, 0, 0 };
			const f3 half = f3_make(0.5f * (float) s.dx, 0.5f * (float) s.dy, 0.5f * (float) s.dz);
			const f3 A = f3_make(d.x * half.x, d.y * half.y, d.z * half.z);
			const f3 B = f3_make(fmaf(o.x, half.x, half.x - 0.5f), fmaf(o.y, half.y, half.y - 0.5f), fmaf(o.z, half.z, half.z - 0.5f));
			const f3 light_pos = f3_make(p->view.light_pos[0], p->view.light_pos[1], p->view.light_pos[2]);
			uint32_t count = 0;
			while (kx <= ky) {
				const float xb = fmaf(kx, A.x, B.x), yb = fmaf(kx, A.y, B.y), zb = fmaf(kx, A.z, B.z);
				const float raw = sample_trilinear_raw(&s, xb, yb, zb);
				f4 cur = tf_linear(&s, raw);
				count++;
				/* the insertion: steps 3 and 4 */
				const uint32_t ix = label_axis(xb, s.dx, perturb), iy = label_axis(yb, s.dy, perturb), iz = label_axis(zb, s.dz, perturb);
				const uint32_t l = labels[((size_t) iz * s.dy + iy) * s.dx + ix];
				const float *e = table + 5 * l;
				if (cur.w > 0.0f) by_label[l]++;
				if (perturb != LABEL_AFTER_SHADING) label_apply(e, perturb, &cur);
				if (cur.w > 0.05f) {
					if (lighting != NULL)
						(void) shade_blinn_phong(&s, lighting, shin, light_pos, d, pt, xb, yb, zb, half, &cur);
					else if (p->light_kd > 0.01f)
						shade_cue(&s, light_pos, pt, xb, yb, zb, half, raw, &cur);
					if (q != NULL) {
						const float sf = shadow_factor(q, S, strength, pt);
						cur.x *= sf; cur.y *= sf; cur.z *= sf;
					}
				}
				if (perturb == LABEL_AFTER_SHADING) label_apply(e, 0, &cur);
				const float t = 1 - acc.w;
				acc.x = fmaf(cur.x, t, acc.x); acc.y = fmaf(cur.y, t, acc.y);
				acc.z = fmaf(cur.z, t, acc.z); acc.w = fmaf(cur.w, t, acc.w);
				if (acc.w > p->ray_threshold)
					break;
				kx += p->ray_step;
				pt = march_point(1, o, d, kx);
			}
			write_pixel(acc, out + 4 * px);
			if (count_out != NULL) count_out[px] = count;
		}
	if (label_count_out != NULL) memcpy(label_count_out, by_label, sizeof by_label);
	return 0;
}
