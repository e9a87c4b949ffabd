/*
 * tf2d_ref.c — the 2D transfer-function frame of include/vr_hip.h (vr_hip_render_tf2d) and the gradient histogram
 * (vr_hip_gradient_histogram) restated with the CPU oracle's own statics.
 * TEST INFRASTRUCTURE: compiled once per session by tests/tf2d_helpers.py through ref_library.compile_test_library, with the flags of
 * tests/feature_ref.c.
 *
 * It includes tests/feature_ref.c read-only, once: the ray is get_ray + intersect + clip_segment, the leaping is first_sample (on the ESL
 * bits the caller built from the envelope), a sample is sample_trilinear_raw at fma(k, A, B), a row's lookup tf_linear on a scene whose
 * transfer function is that row, the gradient field_gradient, the shading shade_cue or shade_blinn_phong (which forms field_gradient of the
 * same arguments again: the same bits), the shadow shadow_factor, the pixel write_pixel.  Its own arithmetic is steps 5 and 6 of the
 * contract (the row and the blend of two rows), the histogram's voxel differences, and the loop that places them.
 *
 * Whole frames only.  clip: the ten floats of vr_clip, never NULL.  lighting NULL = the reference's cue; q NULL = no shadow.
 * table: rows * 128 * 4 floats.
 * perturb: 0 = the contract.  The sensitivity test's wrong readings of it: 1 = the nearest row instead of the interpolated one; 2 = the row
 * from gg instead of g; 3 = the gradient without half_x / y / z; 4 = the row weight rounded to 8 fractional bits as the _Q8 weights are.
 */
#include "feature_ref.c"

enum { TF2D_NEAREST_ROW = 1, TF2D_ROW_FROM_GG = 2, TF2D_NO_HALF = 3, TF2D_WEIGHT_Q8 = 4 };

static float gradient_length(float gx, float gy, float gz, uint32_t perturb) {
	const float gg = fmaf(gz, gz, fmaf(gy, gy, gx * gx));
	if (perturb == TF2D_ROW_FROM_GG) return gg;
	return gg > 0.0f ? gg * rsqrt_nr(gg) : 0.0f;
}

static float row_coordinate(float g, float g_scale, uint32_t rows) {
	const float top = (float) (rows - 1);
	const float v = g * g_scale;
	return v < 0.0f ? 0.0f : (v > top ? top : v);                   /* fmed3(v, 0, rows - 1): v is never NaN (g finite, g_scale finite) */
}

/* out: the frame.  count_out (may be NULL): per pixel the samples of its accumulation loop.  row_count_out (may be NULL): 8 sums over the
 * frame — the samples whose colour has alpha above 0, by lower row j.  kind_count_out (may be NULL): 2 sums — those samples by kind of entry,
 * [0] g-independent, [1] g-dependent (g_dependent: the 128 flags as four words). */
int tf2d_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *table, uint32_t rows, float g_scale,
                const uint32_t *esl, const float *clip, const float *lighting, uint32_t shin, const uint8_t *q, uint32_t S, float strength,
                const uint32_t *g_dependent, uint32_t perturb, uint8_t *out, uint32_t *count_out, uint64_t *row_count_out, uint64_t *kind_count_out) {
	if (!trilinear_mode(p) || perturb > 4 || clip == NULL || table == NULL || rows < 2 || rows > 8)
		return 1;
	const scene s = scene_of(p, voxels, dims, bpv, table, esl);
	uint64_t by_row[8] = { 0 }, by_kind[2] = { 0 };
	memset(out, 0, (size_t) p->out_width * p->out_rows * 4);
	#pragma omp parallel for schedule(dynamic, 4) reduction(+:by_row[:8]) reduction(+:by_kind[:2])
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
			const f3 ones = f3_make(1.0f, 1.0f, 1.0f);
			uint32_t count = 0;
			while (kx <= ky) {
				const float xb = fmaf(kx, A.x, B.x), yb = fmaf(kx, A.y, B.y), zb = fmaf(kx, A.z, B.z);
				const float raw = sample_trilinear_raw(&s, xb, yb, zb);
				count++;
				/* steps 4-6: the gradient, the row, the two rows' lookups and their blend */
				const f3 g3 = field_gradient(&s, xb, yb, zb, perturb == TF2D_NO_HALF ? ones : half);
				const float tg = row_coordinate(gradient_length(g3.x, g3.y, g3.z, perturb), g_scale, rows);
				uint32_t j = (uint32_t) tg;
				if (j > rows - 2) j = rows - 2;
				float wg = tg - (float) j;
				if (perturb == TF2D_NEAREST_ROW) wg = wg < 0.5f ? 0.0f : 1.0f;
				if (perturb == TF2D_WEIGHT_Q8) wg = rintf(wg * 256.0f) * (1.0f / 256.0f);
				scene row = s;
				row.tf = (const f4 *) table + (size_t) j * VR_TF_SIZE;
				const f4 cj = tf_linear(&row, raw);
				row.tf += VR_TF_SIZE;
				const f4 ck = tf_linear(&row, raw);
				f4 cur = { fmaf(wg, ck.x - cj.x, cj.x), fmaf(wg, ck.y - cj.y, cj.y), fmaf(wg, ck.z - cj.z, cj.z), fmaf(wg, ck.w - cj.w, cj.w) };
				if (cur.w > 0.0f) {
					by_row[j]++;
					if (g_dependent != NULL) {
						const float scale = s.bpv == 1 ? (float) VR_TF_SIZE / 255.0f : (float) VR_TF_SIZE / 65535.0f;
						float tb = fmaf(raw, scale, -0.5f);
						tb = tb < 0.0f ? 0.0f : (tb > (float) (VR_TF_SIZE - 1) ? (float) (VR_TF_SIZE - 1) : tb);
						const uint32_t i = (uint32_t) (int) tb;
						by_kind[(g_dependent[i >> 5] >> (i & 31u)) & 1u]++;
					}
				}
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
	if (row_count_out != NULL) memcpy(row_count_out, by_row, sizeof by_row);
	if (kind_count_out != NULL) memcpy(kind_count_out, by_kind, sizeof by_kind);
	return 0;
}

/* step 12 of the contract: hist[g_bins * 256], zeroed here */
int gradient_histogram_ref(const void *voxels, const uint32_t dims[3], uint32_t bpv, uint32_t g_bins, float g_scale, uint64_t *hist) {
	if (g_bins < 1 || g_bins > 32 || (bpv != 1 && bpv != 2))
		return 1;
	const uint8_t *v8 = (const uint8_t *) voxels;
	const uint16_t *v16 = (const uint16_t *) voxels;
	const int64_t nx = dims[0], ny = dims[1], nz = dims[2];
	const float hx = 0.5f * (float) dims[0], hy = 0.5f * (float) dims[1], hz = 0.5f * (float) dims[2];
	memset(hist, 0, (size_t) g_bins * 256 * sizeof(uint64_t));
#define CLAMPED(i, n) ((i) < 0 ? 0 : ((i) > (n) - 1 ? (n) - 1 : (i)))
#define VOXEL(x, y, z) ((float) (bpv == 1 ? (uint32_t) v8[((z) * ny + (y)) * nx + (x)] : (uint32_t) v16[((z) * ny + (y)) * nx + (x)]))
	for (int64_t z = 0; z < nz; z++)
		for (int64_t y = 0; y < ny; y++)
			for (int64_t x = 0; x < nx; x++) {
				const uint32_t raw = (uint32_t) VOXEL(x, y, z);
				const uint32_t bin = bpv == 1 ? raw : raw >> 8;
				const float gx = (VOXEL(CLAMPED(x + 1, nx), y, z) - VOXEL(CLAMPED(x - 1, nx), y, z)) * hx;
				const float gy = (VOXEL(x, CLAMPED(y + 1, ny), z) - VOXEL(x, CLAMPED(y - 1, ny), z)) * hy;
				const float gz = (VOXEL(x, y, CLAMPED(z + 1, nz)) - VOXEL(x, y, CLAMPED(z - 1, nz))) * hz;
				const float tg = row_coordinate(gradient_length(gx, gy, gz, 0), g_scale, g_bins);
				hist[(size_t) (uint32_t) (tg + 0.5f) * 256 + bin]++;
			}
#undef VOXEL
#undef CLAMPED
	return 0;
}
