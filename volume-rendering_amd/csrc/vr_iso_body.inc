// vr_iso_body.inc — the statements of iso_kernel and iso_clipped (vr_project.hip, which includes this text inside both with `constexpr bool CLIP`
// set): a, vol, tf_g, bounds_g, level, refine, out, depth are the kernel's parameters.
	typedef LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)> L;
	constexpr uint32_t kThreads = L::threads;
	constexpr bool kQ8 = SAMPLING == VR_SAMPLE_TRILINEAR_Q8;
	static_assert(SAMPLING != VR_SAMPLE_NEAREST, "a gradient-shaded first hit is defined on the interpolated field");
	__shared__ __attribute__((aligned(16))) uint32_t lut[L::words];
	const bool skipping = a.p.esl != 0u;                            // wave-uniform: a kernel argument
	if constexpr (L::max_dim != 0) stage_brick_tables<BPV, ADDR, LAYOUT>(a, lut);
	if (skipping) {
		// word (z * 32 + y), bit x: the block's dilated bound, widened as mip_kernel widens it, is below the level
		auto widen = [](uint32_t high) { return BPV == 1 ? (float) high : (kQ8 ? (float) ((high + 1u) << 8) : (float) ((high << 8) | 0xffu)); };
		const uint4 *src = (const uint4 *) (bounds_g + kMipBoundEntries);
		for (uint32_t w = threadIdx.x; w < VR_ESL_VOLUME_SIZE; w += kThreads) {
			const uint4 lo16 = src[2u * w], hi16 = src[2u * w + 1u];
			const uint32_t bytes[8] = { lo16.x, lo16.y, lo16.z, lo16.w, hi16.x, hi16.y, hi16.z, hi16.w };
			uint32_t bits = 0u;
			#pragma unroll
			for (uint32_t x = 0; x < 32u; x++) bits |= (widen((bytes[x >> 2] >> (8u * (x & 3u))) & 0xffu) < level ? 1u : 0u) << x;
			iso_skip_lds[w] = bits;
		}
	}
	__syncthreads();

	uint32_t tile_x, tile_y, lx, ly;
	tile_to_xy(a.tiles_x, a.tiles_y, blockIdx.x, blockIdx.x, tile_x, tile_y);
	lane_pixel<kThreads>(a, tile_x, tile_y, lx, ly);
	if (lx >= a.p.out_width || ly >= a.p.out_rows)
		return;                                     // no barrier below this point
	const size_t px = (size_t) ly * a.p.out_width + lx;

	const PixelRay ray = pixel_ray(a, a.p.x0 + lx, frame_row(a, ly));
	f3 origin = ray.origin, dir = ray.dir;
	float kx = ray.kx, ky = ray.ky;
	const float step = a.p.ray_step;
	bool alive = ray.alive;
	if constexpr (CLIP) alive = clip_segment(origin, dir, kx, ky) && alive;
	if (!alive) { kx = 0.0f; ky = 0.0f; origin = mk3(0.0f, 0.0f, 0.0f); dir = origin; }      // lanes without a segment: position 0, never live

	const f3 A = mk3(dir.x * a.half_x, dir.y * a.half_y, dir.z * a.half_z);
	const f3 B = mk3(VR_FMA(origin.x, a.half_x, a.off_x), VR_FMA(origin.y, a.half_y, a.off_y), VR_FMA(origin.z, a.half_z, a.off_z));
	auto fetch_at = [&](float xb, float yb, float zb) { return tri_issue<BPV, ADDR, LAYOUT>(vol, a, lut, xb, yb, zb, true); };
	auto value_of = [&](const TriFetch<BPV, LAYOUT> &f, float xb, float yb, float zb) { return tri_resolve<BPV, LAYOUT, kQ8>(f, a, xb, yb, zb); };
	auto below_level = [&](float k) {
		const BlockIdx b = block_index(a, march_point<SAMPLING>(origin, dir, k));
		return ((iso_skip_lds[b.z * VR_ESL_VOLUME_DIMS + b.y] >> (b.x & 31u)) & 1u) != 0u;
	};

	// -- the march: mip_kernel's two instantiations of the batch, consumed in order; `took` = the lane sampled here (and fetched)
	float k = kx, lo = kx, hi = kx, k_before = kx;
	bool live = alive, found = false;
	auto march = [&](auto skip_tag) {
		constexpr bool kSkip = decltype(skip_tag)::value;
		while (__builtin_amdgcn_ballot_w64(live) != 0ull) {
			TriFetch<BPV, LAYOUT> f[kMipBatch];
			float ks[kMipBatch];
			uint64_t fetched[kMipBatch];
			bool took[kMipBatch];
			#pragma unroll
			for (int u = 0; u < kMipBatch; u++) {
				ks[u] = k;
				if constexpr (kSkip) {
					took[u] = live && !below_level(k);
					f[u].w0 = f[u].w1 = f[u].w2 = f[u].w3 = 0u; f[u].q = 0ull; f[u].q2 = 0ull; f[u].o = (u32x4) (0u);
					fetched[u] = __builtin_amdgcn_ballot_w64(took[u]);
					if (fetched[u] != 0ull) {
						if (took[u]) f[u] = fetch_at(VR_FMA(k, A.x, B.x), VR_FMA(k, A.y, B.y), VR_FMA(k, A.z, B.z));
					}
					k += step;
				} else {
					took[u] = live;
					fetched[u] = ~0ull;
					f[u] = fetch_at(VR_FMA(k, A.x, B.x), VR_FMA(k, A.y, B.y), VR_FMA(k, A.z, B.z));
					k += live ? step : 0.0f;
				}
				live = live && k <= ky;
			}
			__builtin_amdgcn_sched_barrier(0);
			#pragma unroll
			for (int u = 0; u < kMipBatch; u++) {
				if (!kSkip || fetched[u] != 0ull) {     // (a lane that did not fetch resolves zeros: `took` keeps it out)
					const float raw = value_of(f[u], VR_FMA(ks[u], A.x, B.x), VR_FMA(ks[u], A.y, B.y), VR_FMA(ks[u], A.z, B.z));
					if (took[u] && !found && raw >= level) { found = true; hi = ks[u]; lo = u == 0 ? k_before : ks[u > 0 ? u - 1 : 0]; }
				}
			}
			k_before = ks[kMipBatch - 1];
			live = live && !found;
		}
	};
	if (skipping) march(std::true_type()); else march(std::false_type());

	// -- after the loop: bisection, then the gradient, for the waves that hold a surface pixel
	float shade = 1.0f;
	if (__builtin_amdgcn_ballot_w64(found) != 0ull) {
		for (uint32_t r = 0; r < refine; r++) {
			const float mid = 0.5f * (lo + hi);
			const float xb = VR_FMA(mid, A.x, B.x), yb = VR_FMA(mid, A.y, B.y), zb = VR_FMA(mid, A.z, B.z);
			const bool reached = value_of(fetch_at(xb, yb, zb), xb, yb, zb) >= level;
			hi = reached ? mid : hi;
			lo = reached ? lo : mid;
		}
		if (!(a.p.light_kd <= 0.01f)) {
			const float xb = VR_FMA(hi, A.x, B.x), yb = VR_FMA(hi, A.y, B.y), zb = VR_FMA(hi, A.z, B.z);
			const TriFetch<BPV, LAYOUT> fxp = fetch_at(xb + 1.0f, yb, zb), fxm = fetch_at(xb - 1.0f, yb, zb);
			const TriFetch<BPV, LAYOUT> fyp = fetch_at(xb, yb + 1.0f, zb), fym = fetch_at(xb, yb - 1.0f, zb);
			const TriFetch<BPV, LAYOUT> fzp = fetch_at(xb, yb, zb + 1.0f), fzm = fetch_at(xb, yb, zb - 1.0f);
			__builtin_amdgcn_sched_barrier(0);
			const float gx = (value_of(fxp, xb + 1.0f, yb, zb) - value_of(fxm, xb - 1.0f, yb, zb)) * a.half_x;
			const float gy = (value_of(fyp, xb, yb + 1.0f, zb) - value_of(fym, xb, yb - 1.0f, zb)) * a.half_y;
			const float gz = (value_of(fzp, xb, yb, zb + 1.0f) - value_of(fzm, xb, yb, zb - 1.0f)) * a.half_z;
			const float gg = VR_FMA(gz, gz, VR_FMA(gy, gy, gx * gx));
			float s = 0.0f;
			if (gg > 0.0f) {
				const f3 pt = march_point<SAMPLING>(origin, dir, hi);
				const f3 dl = mk3(a.p.view.light_pos[0] - pt.x, a.p.view.light_pos[1] - pt.y, a.p.view.light_pos[2] - pt.z);
				const float il = rsqrt_nr(VR_FMA(dl.z, dl.z, VR_FMA(dl.y, dl.y, dl.x * dl.x)));
				const float dot = VR_FMA(gz, dl.z, VR_FMA(gy, dl.y, gx * dl.x));
				s = __builtin_fminf(__builtin_fabsf((dot * rsqrt_nr(gg)) * il), 1.0f);      // two-sided: lit alike from inside and outside
			}
			shade = VR_FMA(a.p.light_kd, s, 1.0f - a.p.light_kd);
		}
	}

	// -- write_color of the level's filtered transfer-function lookup (the arithmetic of mip_kernel's), shaded; misses store 0 and -1
	uint32_t rgba = 0;
	if (found) {
		const f4 *tf4 = (const f4 *) tf_g;
		const float tb = __builtin_amdgcn_fmed3f(VR_FMA(level, a.tf_scale, -0.5f), 0.0f, (float) (VR_TF_SIZE - 1));
		const uint32_t i = (uint32_t) (int) tb, i1 = i + 1u < VR_TF_SIZE ? i + 1u : i;
		const float w = filter_weight<kQ8>(__builtin_amdgcn_fractf(tb));
		const f4 c0 = tf4[i], c1 = tf4[i1];
		const float cx = VR_FMA(w, c1.x - c0.x, c0.x), cy = VR_FMA(w, c1.y - c0.y, c0.y), cz = VR_FMA(w, c1.z - c0.z, c0.z), cw = VR_FMA(w, c1.w - c0.w, c0.w);
		rgba = map_float_int(cx * shade, 256) | (map_float_int(cy * shade, 256) << 8) | (map_float_int(cz * shade, 256) << 16) | (map_float_int(cw, 256) << 24);
	}
	out[px] = rgba;
	if (depth != nullptr) depth[px] = found ? hi : -1.0f;       // (wave-uniform: a kernel argument)
