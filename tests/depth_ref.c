/*
 * depth_ref.c — the depth frames of include/vr_hip.h (vr_hip_render_depth, vr_hip_pick) restated with the CPU oracle's own statics.
 * TEST INFRASTRUCTURE: compiled once per session by tests/depth_helpers.py through ref_library.compile_test_library, with the flags of
 * tests/feature_ref.c.
 *
 * It includes tests/feature_ref.c read-only, once: the ray is get_ray + intersect + clip_segment, the leaping is first_sample, a sample is
 * sample_trilinear_raw at fma(k, A, B), the alpha is the .w of tf_linear or of slab_colour — the texts the composite restatements
 * (clip_render, slab_render, light_render, shadow_render) are made of.  Its own arithmetic is steps 3 (g and acc), 4 and 5 of the depth
 * contract, and the position and voxel index of a pick, nothing else.
 *
 * Whole frames only.  clip: the ten floats of vr_clip, never NULL (a depth frame always runs the clip's arithmetic: the identity clip when
 * none is set).  cmode: 0 = point classification, 1 = slab classification, 3 = slab_colour's wrong reading "a skipped predecessor is none" (sensitivity;
 * passed to slab_colour unchanged).  mode: vr_depth_mode.
 * perturb: 0 = the contract.  The sensitivity test's wrong readings of it: 1 = FIRST tests acc before the update; 2 = the sample that
 * terminates the ray is not recorded; 3 = MEAN divides by the final alpha; 4 = PEAK takes the last of equal peaks (`g >= best`).
 */
#include "feature_ref.c"

enum { DEPTH_FIRST = 0, DEPTH_PEAK = 1, DEPTH_MEAN = 2 };
enum { DEPTH_ACC_BEFORE = 1, DEPTH_TERMINATOR_LOST = 2, DEPTH_MEAN_BY_ALPHA = 3, DEPTH_PEAK_LAST = 4 };

/* depth_out, value_out, alpha_out: floats.  count_out (may be NULL): per pixel the samples of its accumulation loop, 0 for a ray whose
 * clipped segment is leapt over entirely, 0xfffffffe for a ray that hits the cube and is clipped away, 0xffffffff for a ray that misses
 * the cube.  last_out (may be NULL): k of the last sample of the loop, NaN where there is none; its sign bit is set (-k, k > 0 on every such ray) where that sample terminated the ray.  pick_out (may be
 * NULL): six floats per pixel, position and voxel index of the pick at that pixel, zeros without a hit.  wide_out (may be NULL): samples of
 * the frame that took the wide-slab branch. */
int depth_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl, const float *clip,
                 uint32_t cmode, float opacity, uint32_t mode, uint32_t perturb, float *depth_out, float *value_out, float *alpha_out, uint32_t *count_out,
                 float *last_out, float *pick_out, uint64_t *wide_out) {
	if (!trilinear_mode(p) || (cmode > 1 && cmode != 3) || mode > DEPTH_MEAN || perturb > 4 || clip == NULL)
		return 1;
	const scene s = scene_of(p, voxels, dims, bpv, tf, esl);
	slab_tables tables;
	slab_tables_of(tf, bpv, &tables);
	const features f = { .clip = clip, .mode = cmode, .slab = &tables };
	uint64_t wide = 0;
	#pragma omp parallel for schedule(dynamic, 4) reduction(+:wide)
	for (uint32_t y = 0; y < p->out_rows; y++)
		for (uint32_t x = 0; x < p->out_width; x++) {
			f3 o, d, pt;
			float kx, ky;
			const size_t px = (size_t) y * p->out_width + x;
			depth_out[px] = -1.0f; value_out[px] = -1.0f; alpha_out[px] = 0.0f;
			if (count_out != NULL) count_out[px] = 0xffffffffu;
			if (last_out != NULL) last_out[px] = NAN;
			if (pick_out != NULL) for (int j = 0; j < 6; j++) pick_out[6 * px + j] = 0.0f;
			/* step 1 */
			get_ray(&p->view, (int) x, (int) y, &o, &d);
			if (!intersect(&s, o, d, &kx, &ky))
				continue;
			if (count_out != NULL) count_out[px] = 0xfffffffeu;
			if (!clip_segment(clip, o, d, &kx, &ky))
				continue;
			if (count_out != NULL) count_out[px] = 0;
			/* step 2 */
			if (!first_sample(&s, o, d, &kx, ky, &pt))
				continue;
			/* step 3 */
			const f3 half = f3_make(0.5f * (float) s.dx, 0.5f * (float) s.dy, 0.5f * (float) s.dz);
			const f3 A = f3_make(d.x * half.x, d.y * half.y, d.z * half.z);
			const f3 B = f3_make(fmaf(o.x, half.x, half.x - 0.5f), fmaf(o.y, half.y, half.y - 0.5f), fmaf(o.z, half.z, half.z - 0.5f));
			uint64_t n[N_COUNTERS] = { 0 };
			int first = 1, skipped = 0, found = 0, terminated = 0;
			float tp = 0.0f, acc = 0.0f, best = 0.0f, sg = 0.0f, sk = 0.0f, sv = 0.0f, rk = -1.0f, rv = -1.0f, last = NAN;
			uint32_t count = 0;
			while (kx <= ky) {
				const float raw = sample_trilinear_raw(&s, fmaf(kx, A.x, B.x), fmaf(kx, A.y, B.y), fmaf(kx, A.z, B.z));
				const float a = cmode == 0 ? tf_linear(&s, raw).w : slab_colour(&s, &f, raw, &first, &skipped, &tp, n).w;
				const float before = acc;
				const float t = 1 - acc;
				const float g = a * t;
				acc = fmaf(a, t, acc);
				count++;
				last = kx;
				terminated = acc > p->ray_threshold;
				/* step 4 */
				if (!(perturb == DEPTH_TERMINATOR_LOST && terminated)) {
					if (mode == DEPTH_FIRST) {
						if (!found && (perturb == DEPTH_ACC_BEFORE ? before : acc) >= opacity) { found = 1; rk = kx; rv = raw; }
					} else if (mode == DEPTH_PEAK) {
						if (perturb == DEPTH_PEAK_LAST ? (g >= best) : (g > best)) { best = g; rk = kx; rv = raw; }
					} else {
						sg = sg + g; sk = fmaf(kx, g, sk); sv = fmaf(raw, g, sv);
					}
				}
				if (terminated)
					break;
				kx += p->ray_step;
			}
			wide += n[N_WIDE];
			/* step 5 */
			if (mode == DEPTH_MEAN) {
				const float by = perturb == DEPTH_MEAN_BY_ALPHA ? acc : sg;
				if (sg > 0) { rk = sk / by; rv = sv / by; }
			}
			depth_out[px] = rk; value_out[px] = rv; alpha_out[px] = acc;
			if (count_out != NULL) count_out[px] = count;
			if (last_out != NULL) last_out[px] = terminated ? -last : last;
			/* the pick: position = fma(dir, k, origin) (march_point), voxel = fma(k, A, B) */
			if (pick_out != NULL && rk >= 0.0f) {
				const f3 pos = march_point(1, o, d, rk);
				float *q = pick_out + 6 * px;
				q[0] = pos.x; q[1] = pos.y; q[2] = pos.z;
				q[3] = fmaf(rk, A.x, B.x); q[4] = fmaf(rk, A.y, B.y); q[5] = fmaf(rk, A.z, B.z);
			}
		}
	if (wide_out != NULL) *wide_out = wide;
	return 0;
}
