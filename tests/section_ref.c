/*
 * section_ref.c — the section frames of include/vr_hip.h (vr_hip_render_section, vr_hip_render_section_in_volume) restated with the CPU
 * oracle's own statics.  TEST INFRASTRUCTURE: compiled once per session by tests/section_helpers.py through
 * ref_library.compile_test_library, with the flags of tests/feature_ref.c.
 *
 * It includes tests/feature_ref.c read-only, once: the ray is get_ray + intersect + clip_segment, a sample is sample_trilinear_raw at
 * fma(k, A, B), the transfer-function colour is tf_linear, the pixel is write_pixel, the composite pass of the in-volume frame is
 * backdrop_render.  Its own arithmetic is steps 2, 3, 5, 6 and 7 of the section contract, nothing else.
 *
 * Whole frames only.  clip: the ten floats of vr_clip, never NULL (a section frame always runs the clip's arithmetic: the identity clip
 * when none is set).  section: plane[4], half_width, window lo, window hi — seven floats; mode: vr_section_mode.
 * perturb: 0 = the contract.  The sensitivity test's four wrong readings of it: 1 = a POINT pixel needs kx < kc; 2 = the mean divides by
 * n + 1; 3 = the minimum starts at 0; 4 = the depth of a thick pixel is kc.  5 is no wrong reading but the tie of the modes: a thick mode
 * evaluated on POINT's segment [kc, kc] (half_width is not looked at) — its one sample is the maximum, the minimum and the mean.
 */
#include "feature_ref.c"

enum { SECTION_POINT = 0, SECTION_MAX = 1, SECTION_MIN = 2, SECTION_MEAN = 3 };
enum { SECTION_KX_LT_KC = 1, SECTION_MEAN_N_PLUS_1 = 2, SECTION_MIN_FROM_0 = 3, SECTION_THICK_DEPTH_KC = 4, SECTION_THICK_ON_KC = 5 };

/* step 6 with a window: inv formed once, the difference and the product rounded separately, fmed3(.., 0, 1) for the finite value of a frame */
static float section_grey(float value, float lo, float inv) {
	const float g = (value - lo) * inv;
	return g < 0.0f ? 0.0f : (g > 1.0f ? 1.0f : g);
}

/* out: RGBA8; depth_out: floats; count_out (may be NULL): per pixel the samples of its section, 0 for a ray that hits the cube (under the
 * clip) without a section, 0xffffffff for a ray that misses; value_out (may be NULL): the value of step 5, NaN where there is none */
int section_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const float *clip,
                   const float *section, uint32_t mode, uint32_t perturb, uint8_t *out, float *depth_out, uint32_t *count_out, float *value_out) {
	if (!trilinear_mode(p) || mode > SECTION_MEAN || perturb > 5 || clip == NULL)
		return 1;
	const scene s = scene_of(p, voxels, dims, bpv, tf, NULL);
	const float *n = section, h = section[4], lo = section[5], hi = section[6];
	const int windowed = !(lo == 0.0f && hi == 0.0f);
	const float inv = windowed ? 1.0f / (hi - lo) : 0.0f;
	memset(out, 0, (size_t) p->out_width * p->out_rows * 4);
	#pragma omp parallel for schedule(dynamic, 4)
	for (uint32_t y = 0; y < p->out_rows; y++)
		for (uint32_t x = 0; x < p->out_width; x++) {
			f3 o, d;
			float kx, ky;
			const size_t px = (size_t) y * p->out_width + x;
			depth_out[px] = -1.0f;
			if (count_out != NULL) count_out[px] = 0xffffffffu;
			if (value_out != NULL) value_out[px] = NAN;
			/* step 1 */
			get_ray(&p->view, (int) x, (int) y, &o, &d);
			if (!intersect(&s, o, d, &kx, &ky))
				continue;
			if (!clip_segment(clip, o, d, &kx, &ky))
				continue;
			if (count_out != NULL) count_out[px] = 0;
			/* step 2 */
			const float dn = fmaf(n[2], d.z, fmaf(n[1], d.y, n[0] * d.x));
			const float on = fmaf(n[2], o.z, fmaf(n[1], o.y, fmaf(n[0], o.x, n[3])));
			if (dn == 0)
				continue;
			const float kc = -on / dn;
			/* step 3 */
			float front;
			if (mode == SECTION_POINT || perturb == SECTION_THICK_ON_KC) {
				const int in_front = perturb == SECTION_KX_LT_KC ? (kx < kc) : (kx <= kc);
				if (!(in_front && (kc <= ky)))
					continue;
				kx = kc; ky = kc;
				front = kc;
			} else {
				const float ka = ((-h) - on) / dn, kb = (h - on) / dn;
				kx = flmax(kx, flmin(ka, kb));
				ky = flmin(ky, flmax(ka, kb));
				if (!((kx < ky) && (ky > 0)))
					continue;
				front = perturb == SECTION_THICK_DEPTH_KC ? kc : kx;
			}
			/* steps 4, 5 */
			const f3 half = f3_make(0.5f * (float) s.dx, 0.5f * (float) s.dy, 0.5f * (float) s.dz);
			const f3 A = f3_make(d.x * half.x, d.y * half.y, d.z * half.z);
			const f3 B = f3_make(fmaf(o.x, half.x, half.x - 0.5f), fmaf(o.y, half.y, half.y - 0.5f), fmaf(o.z, half.z, half.z - 0.5f));
			float vmax = 0.0f, vmin = perturb == SECTION_MIN_FROM_0 ? 0.0f : INFINITY, sum = 0.0f;
			uint32_t count = 0;
			float k = kx;
			while (k <= ky) {
				const float raw = sample_trilinear_raw(&s, fmaf(k, A.x, B.x), fmaf(k, A.y, B.y), fmaf(k, A.z, B.z));
				vmax = raw > vmax ? raw : vmax;
				vmin = raw < vmin ? raw : vmin;
				sum = sum + raw;
				count++;
				k += p->ray_step;
			}
			float value = vmax;                     /* MAX; POINT: the one sample */
			if (mode == SECTION_MIN) value = vmin;
			else if (mode == SECTION_MEAN) value = sum / (float) (perturb == SECTION_MEAN_N_PLUS_1 ? count + 1 : count);
			else if (mode == SECTION_POINT) value = sum;        /* 0 + v(kc) = v(kc): the sample itself */
			/* steps 6, 7 */
			f4 c;
			if (windowed) {
				const float g = section_grey(value, lo, inv);
				c.x = c.y = c.z = g; c.w = 1.0f;
			} else {
				c = tf_linear(&s, value);
			}
			write_pixel(c, out + 4 * px);
			depth_out[px] = front;
			if (count_out != NULL) count_out[px] = count;
			if (value_out != NULL) value_out[px] = value;
		}
	return 0;
}

/* The section in the volume: section_render into section_out (may be NULL) and depth_out, then backdrop_render over it into out.  The
 * section pass sees the clip and ignores the shadow, the lighting and the classification mode; the composite pass sees all. */
int section_in_volume_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, const uint32_t *esl,
                             const float *clip, const float *lighting, uint32_t shin, const uint8_t *q, uint32_t S, float strength, uint32_t cmode,
                             const float *section, uint32_t mode, uint32_t perturb, uint8_t *out, float *depth_out, uint8_t *section_out) {
	if (section_render(p, voxels, dims, bpv, tf, clip, section, mode, perturb, out, depth_out, NULL, NULL))
		return 1;
	if (section_out != NULL) memcpy(section_out, out, (size_t) p->out_width * p->out_rows * 4);
	return backdrop_render(p, voxels, dims, bpv, tf, esl, clip, lighting, shin, q, S, strength, cmode, 0, out, depth_out, out);
}
