/*
 * mip_bound_ref.c — the bound argument of the MIP kernel's TRILINEAR fetch skipping, checked sample by sample on
 * the CPU.  TEST INFRASTRUCTURE, compiled by tests/ref_library.py next to tests/feature_ref.c.
 *
 * For every sample of every ray of a whole frame: the block of the sample is formed the way the kernel's block_index does (fused
 * march_point, map_float_int((p + 1) / 2, dim) / block edge, the grid of vro_volume_minmax), the bound is the maximum over the 3x3x3
 * neighbouring blocks widened the way the kernel widens it, the value is the oracle's sample_trilinear_raw.  Returns how many samples
 * exceed their bound (0 = every skip the kernel may take is exact) and the smallest margin seen.
 */
#include "../oracle/vr_oracle.c"

long bound_check(const vr_params *p, const void *voxels, const uint32_t dims[3], uint32_t bpv, double *worst_margin) {
	scene s; s.p = p; s.vox8 = voxels; s.vox16 = voxels; s.dx = dims[0]; s.dy = dims[1]; s.dz = dims[2]; s.bpv = bpv; s.tf = NULL; s.esl = NULL;
	s.min_bound = f3_make(-1,-1,-1); s.line_bits = NULL;
	static uint8_t mm[65536]; uint32_t bd; float bs[3];
	vro_volume_minmax(voxels, dims, bpv, mm, &bd, bs);
	static uint8_t dil[32768];
	for (int z = 0; z < 32; z++) for (int y = 0; y < 32; y++) for (int x = 0; x < 32; x++) {
		uint32_t a = 0;
		for (int dz = -1; dz <= 1; dz++) for (int dy = -1; dy <= 1; dy++) for (int dx = -1; dx <= 1; dx++) {
			int nx = x+dx, ny = y+dy, nz = z+dz; if (nx<0||ny<0||nz<0||nx>31||ny>31||nz>31) continue;
			uint32_t v = mm[2*((nz*32+ny)*32+nx)+1]; if (v > a) a = v; }
		dil[(z*32+y)*32+x] = (uint8_t) a;
	}
	const int q8 = p->sampling == VR_SAMPLE_TRILINEAR_Q8;
	long bad = 0; *worst_margin = 1e30;
	for (uint32_t y = 0; y < p->out_rows; y++) for (uint32_t x = 0; x < p->out_width; x++) {
		f3 o, d; float kx, ky;
		get_ray(&p->view, (int) x, (int) y, &o, &d);
		if (!intersect(&s, o, d, &kx, &ky)) continue;
		const f3 half = f3_make(0.5f * s.dx, 0.5f * s.dy, 0.5f * s.dz);
		const f3 A = f3_make(d.x * half.x, d.y * half.y, d.z * half.z);
		const f3 B = f3_make(fmaf(o.x, half.x, half.x - 0.5f), fmaf(o.y, half.y, half.y - 0.5f), fmaf(o.z, half.z, half.z - 0.5f));
		while (kx <= ky) {
			f3 pos = march_point(1, o, d, kx);
			uint32_t bx = map_float_int((pos.x + 1) * 0.5f, s.dx) / bd, by = map_float_int((pos.y + 1) * 0.5f, s.dy) / bd, bz = map_float_int((pos.z + 1) * 0.5f, s.dz) / bd;
			uint32_t hb = dil[(bz*32+by)*32+bx];
			float bound = bpv == 1 ? (float) hb : (q8 ? (float) ((hb + 1u) << 8) : (float) ((hb << 8) | 0xffu));
			float r = sample_trilinear_raw(&s, fmaf(kx, A.x, B.x), fmaf(kx, A.y, B.y), fmaf(kx, A.z, B.z));
			if (r > bound) bad++;
			if (bound - r < *worst_margin) *worst_margin = bound - r;
			kx += p->ray_step;
		}
	}
	return bad;
}
