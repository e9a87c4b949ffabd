// vr_mip_body.inc — the statements of mip_kernel and mip_clipped (vr_project.hip, which includes this text inside both with `constexpr bool CLIP`
// set): a, vol, tf_g, bounds_g, out are the kernel's parameters.
	typedef LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)> L;
	constexpr uint32_t kThreads = L::threads;
	constexpr bool kNearest = SAMPLING == VR_SAMPLE_NEAREST, kQ8 = SAMPLING == VR_SAMPLE_TRILINEAR_Q8;
	// samples per batch: kMipBatch — three in the clipped index-arithmetic quad-brick kernels of 1-byte voxels, so that every clipped kernel keeps
	// 64 VGPRs (their unclipped twins, the path of volumes beyond 2048 voxels per edge, take 65)
	constexpr int kBatch = CLIP && !kNearest && BPV == 1 && ADDR == kAddrWide && LAYOUT == kLayoutBricked ? 3 : kMipBatch;
	__shared__ __attribute__((aligned(16))) uint32_t lut[L::words];
	const bool skipping = a.p.esl != 0u;                            // wave-uniform: a kernel argument
	uint32_t volume_max = 0u;
	if constexpr (L::max_dim != 0) stage_brick_tables<BPV, ADDR, LAYOUT>(a, lut);
	if (skipping) {
		// (32-bit copies: static LDS in front of the dynamic region may leave its base at any multiple of 4)
		const uint32_t *src = (const uint32_t *) (bounds_g + (kNearest ? 0u : kMipBoundEntries));
		uint32_t *dst = (uint32_t *) mip_bound_lds;
		for (uint32_t i = threadIdx.x; i < kMipBoundEntries / 4u; i += kThreads) dst[i] = src[i];
		volume_max = *(const uint32_t *) (bounds_g + 2u * kMipBoundEntries);
	}
	__syncthreads();

	// -- tile = workgroup id: every ray of a MIP frame without skipping is a full march
	uint32_t tile_x, tile_y, lx, ly;
	tile_to_xy(a.tiles_x, a.tiles_y, blockIdx.x, blockIdx.x, tile_x, tile_y);
	lane_pixel<kThreads>(a, tile_x, tile_y, lx, ly);
	if (lx >= a.p.out_width || ly >= a.p.out_rows)
		return;                                     // no barrier below this point
	uint32_t *out_px = out + (size_t) ly * a.p.out_width + lx;

	const PixelRay ray = pixel_ray(a, a.p.x0 + lx, frame_row(a, ly));
	f3 origin = ray.origin, dir = ray.dir;
	float kx = ray.kx, ky = ray.ky;
	const float step = a.p.ray_step;
	bool alive = ray.alive;
	if constexpr (CLIP) alive = clip_segment(origin, dir, kx, ky) && alive;
	const bool hit = alive;
	if (!alive) { kx = 0.0f; ky = 0.0f; origin = mk3(0.0f, 0.0f, 0.0f); dir = origin; }      // lanes without a segment: position 0, never live

	// -- the march: kMipBatch samples issued, then consumed.  With skipping, `need` is decided against the m of the batch's start: a
	//    smaller m only keeps a fetch that a later one would have made unnecessary.
	float k = kx;
	bool live = alive;
#ifdef VR_MIP_STATS
	uint32_t stat_samples = 0u, stat_fetches = 0u;
#define VR_MIP_COUNT(is_live, is_needed) do { stat_samples += (is_live) ? 1u : 0u; stat_fetches += (is_needed) ? 1u : 0u; } while (0)
#define VR_MIP_COUNT_REST() do { if (live && k <= ky) stat_samples += (uint32_t) ((ky - k) / step) + 1u; } while (0)      /* what a stopped ray leaves out (approximate) */
#else
#define VR_MIP_COUNT(is_live, is_needed) do { } while (0)
#define VR_MIP_COUNT_REST() do { } while (0)
#endif
	f4 colour; colour.x = colour.y = colour.z = colour.w = 0.0f;
	const f4 *tf4 = (const f4 *) tf_g;
	auto bound_index = [&](f3 pos) { const BlockIdx b = block_index(a, pos); return (b.z * VR_ESL_VOLUME_DIMS + b.y) * VR_ESL_VOLUME_DIMS + b.x; };
	// Two instantiations of each loop, like the clamp tags of raymarch_kernel.  Without skipping the batch is straight-line code: every
	// lane fetches — a finished lane where its k stopped, the same cell again — and only the maximum looks at liveness.  With skipping a
	// fetch sits behind the wave's vote and the lane's own need; what it loaded is consumed behind the same vote after the whole batch
	// was issued, so the compiler cannot pull the consumer (and the wait in front of it) up to the load.
	if constexpr (kNearest) {
		auto widen = [](uint32_t high) { return BPV == 1 ? high : ((high << 8) | 0xffu); };
		const uint32_t stop_at = widen(volume_max);
		uint32_t m = 0u;
		auto march = [&](auto skip_tag) {
			constexpr bool kSkip = decltype(skip_tag)::value;
			while (__builtin_amdgcn_ballot_w64(live) != 0ull) {
				uint32_t word[kBatch];
				uint64_t fetched[kBatch];
				bool counts[kBatch];
				#pragma unroll
				for (int u = 0; u < kBatch; u++) {
					const f3 pos = march_point<SAMPLING>(origin, dir, k);
					counts[u] = live;
					if constexpr (kSkip) {
						const bool need = live && widen(mip_bound_lds[bound_index(pos)]) > m;
						fetched[u] = __builtin_amdgcn_ballot_w64(need);
						word[u] = 0u;
						VR_MIP_COUNT(live, need);
						if (fetched[u] != 0ull) {
							if (need) word[u] = sample_nearest<BPV, ADDR, LAYOUT>(vol, a, lut, pos);
						}
						k += step;
					} else {
						fetched[u] = ~0ull;
						word[u] = sample_nearest<BPV, ADDR, LAYOUT>(vol, a, lut, pos);
						k += live ? step : 0.0f;
					}
					live = live && k <= ky;
				}
				__builtin_amdgcn_sched_barrier(0);
				#pragma unroll
				for (int u = 0; u < kBatch; u++) {
					if (!kSkip || fetched[u] != 0ull) {     // (lanes that did not fetch hold 0)
						uint32_t s = voxel_of<BPV, LAYOUT>(word[u]);
						if (!kSkip) s = counts[u] ? s : 0u;
						m = s > m ? s : m;
					}
				}
				if (kSkip && m >= stop_at) { VR_MIP_COUNT_REST(); live = false; }
			}
		};
		if (skipping) march(std::true_type()); else march(std::false_type());
		colour = tf4[(BPV == 1 ? m : (m >> 8)) / VR_TF_RATIO];
	} else {
		const f3 A = mk3(dir.x * a.half_x, dir.y * a.half_y, dir.z * a.half_z);
		const f3 B = mk3(VR_FMA(origin.x, a.half_x, a.off_x), VR_FMA(origin.y, a.half_y, a.off_y), VR_FMA(origin.z, a.half_z, a.off_z));
		auto widen = [](uint32_t high) { return BPV == 1 ? (float) high : (kQ8 ? (float) ((high + 1u) << 8) : (float) ((high << 8) | 0xffu)); };
		const float stop_at = widen(volume_max);
		float m = 0.0f;
		auto march = [&](auto skip_tag) {
			constexpr bool kSkip = decltype(skip_tag)::value;
			while (__builtin_amdgcn_ballot_w64(live) != 0ull) {
				TriFetch<BPV, LAYOUT> f[kBatch];
				float ks[kBatch];
				uint64_t fetched[kBatch];
				bool counts[kBatch];
				#pragma unroll
				for (int u = 0; u < kBatch; u++) {
					ks[u] = k;
					counts[u] = live;
					if constexpr (kSkip) {
						const bool need = live && widen(mip_bound_lds[bound_index(march_point<SAMPLING>(origin, dir, k))]) > m;
						f[u].w0 = f[u].w1 = f[u].w2 = f[u].w3 = 0u; f[u].q = 0ull; f[u].q2 = 0ull; f[u].o = (u32x4) (0u);
						fetched[u] = __builtin_amdgcn_ballot_w64(need);
						VR_MIP_COUNT(live, need);
						if (fetched[u] != 0ull) {
							if (need) f[u] = tri_issue<BPV, ADDR, LAYOUT>(vol, a, lut, VR_FMA(k, A.x, B.x), VR_FMA(k, A.y, B.y), VR_FMA(k, A.z, B.z), true);
						}
						k += step;
					} else {
						fetched[u] = ~0ull;
						f[u] = tri_issue<BPV, ADDR, LAYOUT>(vol, a, lut, VR_FMA(k, A.x, B.x), VR_FMA(k, A.y, B.y), VR_FMA(k, A.z, B.z), true);
						k += live ? step : 0.0f;
					}
					live = live && k <= ky;
				}
				__builtin_amdgcn_sched_barrier(0);
				#pragma unroll
				for (int u = 0; u < kBatch; u++) {
					if (!kSkip || fetched[u] != 0ull) {     // (lanes that did not fetch resolve zeros to 0: m >= 0 keeps them unchanged)
						const float raw = tri_resolve<BPV, LAYOUT, kQ8>(f[u], a, VR_FMA(ks[u], A.x, B.x), VR_FMA(ks[u], A.y, B.y), VR_FMA(ks[u], A.z, B.z));
						m = ((kSkip || counts[u]) && raw > m) ? raw : m;
					}
				}
				if (kSkip && m >= stop_at) { VR_MIP_COUNT_REST(); live = false; }
			}
		};
		if (skipping) march(std::true_type()); else march(std::false_type());
		// the filtered lookup of a DVR sample (raymarch_kernel; GPURenderer4.cu:77): entries floor(tb) and floor(tb) + 1, clamp addressing
		const float tb = __builtin_amdgcn_fmed3f(VR_FMA(m, a.tf_scale, -0.5f), 0.0f, (float) (VR_TF_SIZE - 1));
		const uint32_t i = (uint32_t) (int) tb, i1 = i + 1u < VR_TF_SIZE ? i + 1u : i;
		const float w = filter_weight<kQ8>(__builtin_amdgcn_fractf(tb));
		const f4 c0 = tf4[i], c1 = tf4[i1];
		colour.x = VR_FMA(w, c1.x - c0.x, c0.x); colour.y = VR_FMA(w, c1.y - c0.y, c0.y);
		colour.z = VR_FMA(w, c1.z - c0.z, c0.z); colour.w = VR_FMA(w, c1.w - c0.w, c0.w);
	}

	// -- RaycasterBase.h:44-50 write_color of the entry as it is stored (+ the fused clear: misses store 0)
	uint32_t rgba = 0;
	if (hit) {
		rgba = map_float_int(colour.x, 256) | (map_float_int(colour.y, 256) << 8) |
		       (map_float_int(colour.z, 256) << 16) | (map_float_int(colour.w, 256) << 24);
	}
	*out_px = rgba;
#ifdef VR_MIP_STATS
	if (skipping) {
		atomicAdd((unsigned long long *) (bounds_g + kMipStatsAt), (unsigned long long) stat_samples);
		atomicAdd((unsigned long long *) (bounds_g + kMipStatsAt + 8u), (unsigned long long) stat_fetches);
	}
#endif
#undef VR_MIP_COUNT
#undef VR_MIP_COUNT_REST
