/*
 * mip_ref.c — the maximum-intensity projection of include/vr_hip.h (vr_hip_render_mip) restated with the CPU oracle's own statics.
 * TEST INFRASTRUCTURE: compiled on demand by tests/mip_helpers.py with the flags oracle/Makefile uses for libvr_oracle.so.
 *
 * It includes oracle/vr_oracle.c read-only and has no arithmetic of its own: the ray is get_ray + intersect, the sample sequence is
 * the oracle's march with leaping off (k accumulated by repeated addition, the position formed from k), a sample is sample_nearest
 * at march_point or sample_trilinear_raw at fma(k, A, B), the colour is transfer_fn[s8 / TF_RATIO] or tf_linear, the pixel is
 * map_float_int of the colour.  tests/test_mip_model.py pins this file against the unmodified oracle.
 *
 * Whole frames only (pixel (x, y) of the view -> out[y * out_width + x]); raw_out receives the per-pixel maximum — the integer for
 * NEAREST, the bits of the float for TRILINEAR — and 0xffffffff for rays that miss the volume.
 */
#include "../oracle/vr_oracle.c"

int mip_render(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, const float *tf, uint8_t *out, uint32_t *raw_out) {
	scene s;
	s.p = p; s.vox8 = (const uint8_t *) voxels; s.vox16 = (const uint16_t *) voxels;
	s.dx = dims[0]; s.dy = dims[1]; s.dz = dims[2]; s.bpv = bpv;
	s.tf = (const f4 *) tf; s.esl = NULL; s.min_bound = f3_make(-1, -1, -1); s.line_bits = NULL;
	memset(out, 0, (size_t) p->out_width * p->out_rows * 4);
	for (uint32_t y = 0; y < p->out_rows; y++)
		for (uint32_t x = 0; x < p->out_width; x++) {
			f3 o, d;
			float kx, ky;
			const size_t px = (size_t) y * p->out_width + x;
			raw_out[px] = 0xffffffffu;
			get_ray(&p->view, (int) x, (int) y, &o, &d);
			if (!intersect(&s, o, d, &kx, &ky))
				continue;
			const int fused = p->sampling != VR_SAMPLE_NEAREST;
			const f3 half = f3_make(0.5f * (float) s.dx, 0.5f * (float) s.dy, 0.5f * (float) s.dz);
			const f3 A = f3_make(d.x * half.x, d.y * half.y, d.z * half.z);
			const f3 B = f3_make(fmaf(o.x, half.x, half.x - 0.5f), fmaf(o.y, half.y, half.y - 0.5f), fmaf(o.z, half.z, half.z - 0.5f));
			uint32_t mi = 0;
			float mf = 0.0f;
			while (kx <= ky) {
				if (!fused) {
					const uint32_t v = sample_nearest(&s, march_point(0, o, d, kx));
					if (v > mi) mi = v;
				} else {
					const float r = sample_trilinear_raw(&s, fmaf(kx, A.x, B.x), fmaf(kx, A.y, B.y), fmaf(kx, A.z, B.z));
					if (r > mf) mf = r;
				}
				kx += p->ray_step;
			}
			f4 c;
			if (!fused) {
				const uint32_t s8 = bpv == 1 ? mi : mi >> 8;
				c = s.tf[s8 / VR_TF_RATIO];
				raw_out[px] = mi;
			} else {
				c = tf_linear(&s, mf);
				memcpy(&raw_out[px], &mf, 4);
			}
			out[4 * px + 0] = (uint8_t) map_float_int(c.x, 256); out[4 * px + 1] = (uint8_t) map_float_int(c.y, 256);
			out[4 * px + 2] = (uint8_t) map_float_int(c.z, 256); out[4 * px + 3] = (uint8_t) map_float_int(c.w, 256);
		}
	return 0;
}
