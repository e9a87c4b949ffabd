/*
 * fused_ref.c — the fused frame of include/vr_hip.h (vr_hip_render_fused) restated with the CPU oracle's own statics.
 * TEST INFRASTRUCTURE: compiled once per session by tests/fused_helpers.py through ref_library.compile_test_library, with the flags of
 * tests/feature_ref.c.
 *
 * It includes tests/feature_ref.c read-only, once: the ray is get_ray + intersect + clip_segment, the leaping is first_sample (on the ESL
 * bits the caller gives: the fused frame's own), a sample of either field is sample_trilinear_raw at fma(k, A, B) on a scene whose voxels
 * are that field's, its lookup tf_linear on a scene whose transfer function is that field's, field A's shading shade_cue or
 * shade_blinn_phong, the shadow shadow_factor, the pixel write_pixel.  Its own arithmetic is steps 4-7 of the contract: B's sample and
 * lookup, the weights, the two modes, and the loop that places them.
 *
 * Whole frames only.  clip: the ten floats of vr_clip, never NULL.  lighting NULL = the reference's cue; q NULL = no shadow.
 * perturb: 0 = the contract.  The sensitivity test's wrong readings of it: 1 = B shaded with A's cue (the cue's term added to cB as well);
 * 2 = the weight applied in front of A's dense test; 3 = OVER with B in front; 4 = OVER with a termination test between the two
 * accumulations; 5 = SUM as two accumulations with one weight t instead of the product, the fma and one accumulation; 6 = B sampled at its
 * nearest voxel.
 */
#include "feature_ref.c"

enum { FUSED_B_CUE = 1, FUSED_WEIGHT_BEFORE_DENSE = 2, FUSED_B_IN_FRONT = 3, FUSED_TERMINATE_BETWEEN = 4, FUSED_SUM_TWO_FMAS = 5, FUSED_B_NEAREST = 6 };

static f4 f4_times(f4 c, float w) {
	const f4 r = { c.x * w, c.y * w, c.z * w, c.w * w };
	return r;
}

static f4 f4_over(f4 c, f4 acc) {
	const float t = 1 - acc.w;
	const f4 r = { fmaf(c.x, t, acc.x), fmaf(c.y, t, acc.y), fmaf(c.z, t, acc.z), fmaf(c.w, t, acc.w) };
	return r;
}

/* out: the frame.  count_out (may be NULL): per pixel the samples of its accumulation loop.  kind_count_out (may be NULL): 4 sums over the
 * frame — the samples of the loops by which field contributed an alpha above 0 after its weight: [0] none, [1] A only, [2] B only, [3] both.
 * acc_out (may be NULL): per pixel the four accumulated floats the bytes are made of — where two readings differ by roundings alone, few bytes show it. */
int fused_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl, const float *clip,
                 const float *lighting, uint32_t shin, const uint8_t *q, uint32_t S, float strength, const void *voxels_b, const float *tf_b,
                 uint32_t mode, float weight_a, float weight_b, uint32_t perturb, uint8_t *out, uint32_t *count_out, uint64_t *kind_count_out, float *acc_out) {
	if (!trilinear_mode(p) || perturb > 6 || mode > 1 || clip == NULL || voxels_b == NULL || tf_b == NULL)
		return 1;
	const scene s = scene_of(p, voxels, dims, bpv, tf, esl);
	const scene sb = scene_of(p, voxels_b, dims, bpv, tf_b, esl);
	uint64_t by_kind[4] = { 0 };
	memset(out, 0, (size_t) p->out_width * p->out_rows * 4);
	if (acc_out != NULL) memset(acc_out, 0, (size_t) p->out_width * p->out_rows * 4 * sizeof(float));
	#pragma omp parallel for schedule(dynamic, 4) reduction(+:by_kind[:4])
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
				count++;
				/* step 3: field A, the composite's sample */
				const float raw = sample_trilinear_raw(&s, xb, yb, zb);
				f4 ca = tf_linear(&s, raw);
				float cue = 0.0f;
				if (perturb == FUSED_WEIGHT_BEFORE_DENSE ? ca.w * weight_a > 0.05f : ca.w > 0.05f) {
					if (lighting != NULL)
						(void) shade_blinn_phong(&s, lighting, shin, light_pos, d, pt, xb, yb, zb, half, &ca);
					else if (p->light_kd > 0.01f) {
						const float before = ca.x;
						shade_cue(&s, light_pos, pt, xb, yb, zb, half, raw, &ca);
						cue = ca.x - before;
					}
					if (q != NULL) {
						const float sf = shadow_factor(q, S, strength, pt);
						ca.x *= sf; ca.y *= sf; ca.z *= sf;
					}
				}
				/* step 4: field B, emissive */
				const float raw_b = perturb == FUSED_B_NEAREST ? (float) sample_nearest(&sb, pt) : sample_trilinear_raw(&sb, xb, yb, zb);
				f4 cb = tf_linear(&sb, raw_b);
				if (perturb == FUSED_B_CUE) { cb.x += cue; cb.y += cue; cb.z += cue; }
				/* step 5: the weights */
				const f4 wa = f4_times(ca, weight_a);
				by_kind[(wa.w > 0.0f ? 1 : 0) + (cb.w * weight_b > 0.0f ? 2 : 0)]++;
				int stop = 0;
				if (mode == 0 && perturb == FUSED_SUM_TWO_FMAS) {
					const float t = 1 - acc.w;
					const f4 wb = f4_times(cb, weight_b);
					acc.x = fmaf(wb.x, t, fmaf(wa.x, t, acc.x)); acc.y = fmaf(wb.y, t, fmaf(wa.y, t, acc.y));
					acc.z = fmaf(wb.z, t, fmaf(wa.z, t, acc.z)); acc.w = fmaf(wb.w, t, fmaf(wa.w, t, acc.w));
				} else if (mode == 0) {
					/* step 6: VR_FUSE_SUM */
					const f4 c = { fmaf(cb.x, weight_b, wa.x), fmaf(cb.y, weight_b, wa.y), fmaf(cb.z, weight_b, wa.z), fmaf(cb.w, weight_b, wa.w) };
					acc = f4_over(c, acc);
				} else {
					/* step 7: VR_FUSE_OVER */
					const f4 wb = f4_times(cb, weight_b);
					const f4 front = perturb == FUSED_B_IN_FRONT ? wb : wa, back = perturb == FUSED_B_IN_FRONT ? wa : wb;
					acc = f4_over(front, acc);
					if (perturb == FUSED_TERMINATE_BETWEEN && acc.w > p->ray_threshold) stop = 1;
					else acc = f4_over(back, acc);
				}
				if (stop || acc.w > p->ray_threshold)
					break;
				kx += p->ray_step;
				pt = march_point(1, o, d, kx);
			}
			write_pixel(acc, out + 4 * px);
			if (count_out != NULL) count_out[px] = count;
			if (acc_out != NULL) { acc_out[4 * px] = acc.x; acc_out[4 * px + 1] = acc.y; acc_out[4 * px + 2] = acc.z; acc_out[4 * px + 3] = acc.w; }
		}
	if (kind_count_out != NULL) memcpy(kind_count_out, by_kind, sizeof by_kind);
	return 0;
}
