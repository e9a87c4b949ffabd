/*
 * iso_ref.c — the shaded isosurface with depth of include/vr_hip.h (vr_hip_render_iso) restated with the CPU oracle's own statics.
 * TEST INFRASTRUCTURE: compiled on demand by tests/iso_helpers.py with the flags oracle/Makefile uses for libvr_oracle.so.
 *
 * It includes oracle/vr_oracle.c read-only.  The ray is get_ray + intersect, the sample sequence is the oracle's march with leaping off
 * (k accumulated by repeated addition), a field value is sample_trilinear_raw at fma(k, A, B), the base colour is tf_linear of the level,
 * the light vector is normalised with rsqrt_nr at march_point, the pixel is map_float_int of the shaded colour.  Its own arithmetic is
 * the bisection (step 4 of the contract) and the gradient shading (step 6), nothing else.
 *
 * Whole frames only (pixel (x, y) of the view -> out[y * out_width + x]).  depth_out: k* or -1.  counters_out[3]: samples of the march,
 * fetches of the march, surface pixels.  dilated: NULL, or the 32^3 3x3x3-dilated block maxima (high bytes for 2-byte voxels, built on the
 * host as tests/mip_bound_ref.c builds them) and the block edge: the march then skips the fetch of every sample whose widened bound is
 * below the level, as the kernel may — a skipped sample counts as "below the level" without being looked at.
 */
#include "../oracle/vr_oracle.c"

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

int iso_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, float level, uint32_t refine,
               const uint8_t *dilated, uint32_t block_dims, uint8_t *out, float *depth_out, uint64_t *counters_out) {
	if (p->sampling != VR_SAMPLE_TRILINEAR && p->sampling != VR_SAMPLE_TRILINEAR_Q8)
		return 1;
	scene s;
	s.p = p; s.vox8 = (const uint8_t *) voxels; s.vox16 = (const uint16_t *) voxels;
	s.dx = dims[0]; s.dy = dims[1]; s.dz = dims[2]; s.bpv = bpv;
	s.tf = (const f4 *) tf; s.esl = NULL; s.min_bound = f3_make(-1, -1, -1); s.line_bits = NULL;
	const int q8 = p->sampling == VR_SAMPLE_TRILINEAR_Q8;
	const f3 half = f3_make(0.5f * (float) s.dx, 0.5f * (float) s.dy, 0.5f * (float) s.dz);
	const f3 light_pos = f3_make(p->view.light_pos[0], p->view.light_pos[1], p->view.light_pos[2]);
	const f4 base = tf_linear(&s, level);
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
			if (!intersect(&s, o, d, &kx, &ky))
				continue;
			const f3 A = f3_make(d.x * half.x, d.y * half.y, d.z * half.z);
			const f3 B = f3_make(fmaf(o.x, half.x, half.x - 0.5f), fmaf(o.y, half.y, half.y - 0.5f), fmaf(o.z, half.z, half.z - 0.5f));
#define V_AT(k) sample_trilinear_raw(&s, fmaf((k), A.x, B.x), fmaf((k), A.y, B.y), fmaf((k), A.z, B.z))
			/* steps 2, 3: the first sample at or above the level */
			int found = 0, first = 1;
			float lo = kx, hi = kx;
			while (kx <= ky) {
				int fetch = 1;
				samples++;
				if (dilated != NULL) {
					const f3 pos = march_point(1, o, d, kx);
					const uint32_t bx = map_float_int((pos.x + 1) * 0.5f, s.dx) / block_dims, by = map_float_int((pos.y + 1) * 0.5f, s.dy) / block_dims,
					               bz = map_float_int((pos.z + 1) * 0.5f, s.dz) / block_dims;
					const uint32_t hb = dilated[(bz * 32 + by) * 32 + bx];
					const float bound = bpv == 1 ? (float) hb : (q8 ? (float) ((hb + 1u) << 8) : (float) ((hb << 8) | 0xffu));
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
			depth_out[px] = hi;
			/* step 6: two-sided diffuse shading from central differences one texel apart */
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
	counters_out[0] = samples; counters_out[1] = fetches; counters_out[2] = hits;
	return 0;
}
