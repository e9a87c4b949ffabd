// vr_raymarch_body.inc — the statements of the composite-march kernels: vr_composite_family.inc, the one kernel definition, includes this
// text with `constexpr bool CLIP`, `SHADOW`, `LIT`, `SLAB` and `BACKDROP` set as the family says — raymarch_kernel and raymarch_clipped
// (vr_raymarch.hip), raymarch_shadowed (vr_shadow.hip), composite_lit (vr_light.hip), composite_slab and composite_slab_lit (vr_slab.hip),
// the four composite_backdrop* kernels (vr_backdrop.hip, vr_backdrop_slab.hip).  a, vol, tf_g, esl_g, out, tile_order, tile_cost are the kernel's parameters.
	// tile_order: workgroup id -> tile number (measured-cost launch order), or NULL: identity.  tile_cost: per tile, the longest wave of
	// the tile in 64-cycle units (atomicMax), or NULL: not recorded.  Both are consumed FIRST, before the tables are staged: the hot
	// variants sit at the 80-SGPR limit of 8 waves per SIMD and their peak is the staging code, so nothing of the schedule may be live
	// there or during the march — the workgroup's start time and the address of its tile's cost word wait in LDS (one record per
	// workgroup, written by thread 0 before the staging barrier) for the end of every wave.  (A per-wave record indexed by the wave's
	// hardware slot, HW_ID, was tried and is WRONG: a wave that is context-switched out and back — several queues share the GPU —
	// comes back in another slot, reads a record nobody wrote, and the atomic below goes to a wild address.)
	__shared__ uint32_t group_sched[4];
	const uint32_t order_entry = tile_order ? tile_order[blockIdx.x] : blockIdx.x;
	// kLayoutRunDual: bit 31 of the entry selects the tile's copy (runs along y instead of z); it waits in LDS like the rest of the record
	const uint32_t tile_of_group = LAYOUT == kLayoutRunDual ? (order_entry & ~kTileAltBit) : order_entry;
	typedef LutCfg<(LAYOUT != kLayoutLinear ? ADDR : kAddrWide)> L;
	constexpr uint32_t kThreads = L::threads;
	// kLayoutRunDual: which of the two run copies this tile reads.  From the launch-order entry (measured choice, testing aid), or —
	// the product's rule, no history needed — from the bit the HOST set for the tile's group of 64 consecutive tile numbers, i.e. its
	// 8x8-tile block (RayKernelArgs::dual_bits: the analytic entry-face rule of vr_hip_api.cpp dual_choice_bits).  Read through a laundered pointer to the kernel-argument segment
	// (`a` is the first argument: offset 0) so that nothing of it stays in scalar registers across the staging code.
	bool alt_tile = LAYOUT == kLayoutRunDual && (order_entry & kTileAltBit) != 0u;
	if (LAYOUT == kLayoutRunDual && a.dual_analytic != 0u) {
		typedef const RayKernelArgs __attribute__((address_space(4))) *ConstArgs;      // constant address space: scalar loads
		ConstArgs q = (ConstArgs) __builtin_amdgcn_kernarg_segment_ptr();
		asm volatile("" : "+s"(q));
		const uint32_t bit = tile_of_group >> q->dual_shift;        // groups of consecutive tile NUMBERS: 64 = one 8x8-tile block of the numbering
		const uint32_t word = q->dual_bits[(bit >> 5) & (kDualWords - 1u)];
		alt_tile = __builtin_amdgcn_readfirstlane((int) ((word >> (bit & 31u)) & 1u)) != 0;       // uniform by construction (kernel arguments and the tile number only)
	}
	if (threadIdx.x == 0) {
#ifdef VR_BOUNDS_CHECK
		if (tile_of_group >= a.bc_ntiles) { bc_report(a, kBcCostSlot, tile_of_group, a.bc_ntiles); tile_cost = nullptr; }
#endif
		const uint64_t slot = tile_cost ? (uint64_t) (uintptr_t) (tile_cost + tile_of_group) : 0ull;
		group_sched[0] = (uint32_t) (__builtin_readcyclecounter() >> 6); group_sched[1] = (uint32_t) slot; group_sched[2] = (uint32_t) (slot >> 32);
		group_sched[3] = alt_tile ? 1u : 0u;
	}
	constexpr bool kQ8 = SAMPLING == VR_SAMPLE_TRILINEAR_Q8;        // 8-bit filter weights; everything else as TRILINEAR
	constexpr bool kUseLut = L::max_dim != 0;
	__shared__ LdsTables lds;
	__shared__ __attribute__((aligned(16))) uint32_t lut[L::words];
	// SLAB (vr_hip_set_preintegration): the running integral K of the piecewise-linear transfer function, 2 KiB that only the slab kernels
	// declare (one element elsewhere, never referenced: it takes no LDS).  The host uploads K behind the 128 entries of the transfer function.
	__shared__ f4 slab_k[SLAB ? VR_TF_SIZE : 1];
#ifdef VR_LDS_PAD          // tuning aid: occupy extra LDS to lower the number of resident workgroups per CU
	__shared__ uint32_t lds_pad[VR_LDS_PAD / 4];
	if (a.dim_x == 0xffffffffu) lds_pad[threadIdx.x] = 1;
#endif

	// -- stage TF (+ deltas), the ESL bit-volume and the brick address tables in LDS
	{
		const uint32_t t = threadIdx.x;
		if (kUseLut && is_run_layout(LAYOUT)) {
			// r = the run axis (z, or y for kLayoutRunY), o = the other column axis (y, or z); bricks: x fastest, then o, then r.
			// kLayoutRunDual: a tile that reads the copy along y builds ITS tables exactly like kLayoutRunY and marches with the
			// y and z components of its texel-space ray exchanged — the table regions then meet the coordinates they were built for.
			const bool along_y = LAYOUT == kLayoutRunY || alt_tile;
			const uint32_t nx = a.dim_x, nr = along_y ? a.dim_y : a.dim_z, no = along_y ? a.dim_z : a.dim_y;
			const uint32_t nbo = along_y ? a.nbz : a.nby;
			// the flavour of the copies (wave-uniform, vr_device.h): 36-byte runs of 8 cells, or aligned 32-byte runs of SEVEN cells — a
			// cell's table entries say where it lies either way, and nothing below the barrier knows the difference
			const bool aligned = a.run_aligned != 0u;
			const uint32_t run_bytes = aligned ? kRun7Bytes : kRunBytes, brick_bytes = aligned ? kRun7BrickBytes : kRunBrickBytes;
			const uint64_t slab = (uint64_t) a.nbx * nbo * brick_bytes;
			const uint64_t copy_base = alt_tile ? a.alt_copy : (uint64_t) (uintptr_t) vol;
#ifdef VR_BOUNDS_CHECK
			if (t == 0) { bc_table_entries[0] = nx + 2 * kLutPad; bc_table_entries[1] = no + 2 * kLutPad; bc_table_entries[2] = nr + 2 * kLutPad; }
#endif
			for (uint32_t j = t; j < nr + 2 * kLutPad; j += kThreads) {
				const uint32_t i = lut_cell_of(j, nr);
				const uint32_t brick = aligned ? i / kRun7Cells : i >> 3, in_run = aligned ? i - brick * kRun7Cells : i & 7u;
				const uint64_t z0 = copy_base + brick * slab + in_run * 4u;
				lut[2 * j] = (uint32_t) z0; lut[2 * j + 1] = (uint32_t) (z0 >> 32);
			}
			for (uint32_t j = t; j < nx + 2 * kLutPad; j += kThreads) { const uint32_t i = lut_cell_of(j, nx); lut[L::x_at + j] = (i >> 3) * brick_bytes + run_cell_order(0, i & 7u) * run_bytes; }
			for (uint32_t j = t; j < no + 2 * kLutPad; j += kThreads) { const uint32_t i = lut_cell_of(j, no); lut[L::y_at + j] = (i >> 3) * a.nbx * brick_bytes + run_cell_order(1, i & 7u) * run_bytes; }
		} else if constexpr (kUseLut) stage_brick_tables<BPV, ADDR, LAYOUT>(a, lut);      // (kUseLut: not the linear array, so L is LutCfg<ADDR>)
		if (t <= VR_TF_SIZE) {
			const f4 *tf4 = (const f4 *) tf_g;
			uint32_t i0 = t < VR_TF_SIZE ? t : VR_TF_SIZE - 1;
			uint32_t i1 = t + 1 < VR_TF_SIZE ? t + 1 : VR_TF_SIZE - 1;
			f4 c0 = tf4[i0], c1 = tf4[i1];
			lds.tf[t] = c0;
			f4 d; d.x = c1.x - c0.x; d.y = c1.y - c0.y; d.z = c1.z - c0.z; d.w = c1.w - c0.w;
			lds.dtf[t] = d;
		}
		if (SLAB && t < VR_TF_SIZE) slab_k[t] = ((const f4 *) tf_g)[VR_TF_SIZE + t];
		for (uint32_t i = t; i < VR_ESL_VOLUME_SIZE; i += kThreads) lds.esl[i] = esl_g[i];
		if (SAMPLING == VR_SAMPLE_NEAREST && BPV == 1 && t < 256u) lds.unit[t] = (float) t / 255.0f;   // the same IEEE division, once
	}
	__syncthreads();

	uint32_t tile_x, tile_y;
	tile_to_xy(a.tiles_x, a.tiles_y, tile_of_group, blockIdx.x, tile_x, tile_y);

	uint32_t lx, ly;
	lane_pixel<kThreads>(a, tile_x, tile_y, lx, ly);
	if (lx >= a.p.out_width || ly >= a.p.out_rows)
		return;                                     // no barrier below this point
	const uint32_t lane = threadIdx.x & 63u;
	// BACKDROP: the pixel's element index alone crosses the march (one register; out_width * out_rows < 2^32) — the output address and the
	// layer's are formed from it behind the march, from addresses read again in the kernel-argument segment
	uint32_t *out_px = BACKDROP ? nullptr : out + (size_t) ly * a.p.out_width + lx;
	uint32_t pixel = 0;
	if constexpr (BACKDROP) { pixel = ly * a.p.out_width + lx; asm volatile("" : "+v"(pixel)); }

	const PixelRay ray = pixel_ray(a, a.p.x0 + lx, frame_row(a, ly));
	f3 origin = ray.origin, dir = ray.dir;
	float kx = ray.kx, ky = ray.ky;
	const float step = a.p.ray_step;
	bool alive = ray.alive;
	if constexpr (CLIP) alive = clip_segment(origin, dir, kx, ky) && alive;
	// BACKDROP (vr_hip_render_backdrop, DESIGN.md section 4.11): the ray stops at the depth of the opaque layer — k of the pixel's own ray;
	// negative or NaN = no surface (an ordered compare).  Only the narrowed ky crosses the march: the layer is read again behind it.
	if constexpr (BACKDROP) {
		const float d = backdrop_depth_at(pixel);
		if (d >= 0.0f) {
			ky = flmin(ky, d);
			alive = alive && (kx < ky) && (ky > 0);
		}
	}
	const bool hit = alive;
	f3 pt = march_point<SAMPLING>(origin, dir, kx);

	// -- empty space leaping loop (CPURenderer.cpp:18-25)
	// Cooperative look-ahead for zero-leap chains (round 4).  A ray that runs exactly along a block face (rows / columns of pixels of the
	// axis-aligned views; a few rays of every view) finds its block empty but its distance to the exit plane 0 at EVERY sample: it leaps by
	// floor(0 / step) * step = 0 and probes again one step on — up to ~1000 dependent probes by one or two lanes of a wave that is alone
	// on its SIMD at the end of the frame (the default mode's tail).  While at most VR_ESL_COOP_LANES lanes still probe and one of them
	// has just leapt by exactly 0, the whole wave evaluates that ray's next positions — the j-th active lane the position j rounds of
	// "+= 0; += step" on, formed EXACTLY (inside a binade fl(k + step) = k + round_u(step): an arithmetic progression, see ColBatch;
	// else by the sequential additions) — and the ray jumps to the first position whose probe is not again "empty block, zero leap",
	// which the ordinary step below then evaluates.  Exact by construction.
#ifndef VR_ESL_COOP_LANES
#define VR_ESL_COOP_LANES 8
#endif
	if (a.p.esl) {
		bool probing = alive;
		uint64_t zero_leap = 0ull, pm;                                  // lanes whose last probe leapt by exactly 0
		int coop_pause = 0;                                             // a look-ahead that skipped fewer than four positions cost more than it saved: pause (perspective views: their chains are short)
		while ((pm = __builtin_amdgcn_ballot_w64(probing)) != 0ull) {
			const uint64_t chain = pm & zero_leap;
			if (coop_pause > 0) coop_pause--;
			else if (VR_ESL_COOP_LANES > 0 && chain != 0ull && __builtin_popcountll(pm) <= VR_ESL_COOP_LANES) {
				const int leader = __builtin_ctzll(chain);
				const f3 lo = mk3(rlane(origin.x, leader), rlane(origin.y, leader), rlane(origin.z, leader)), ld = mk3(rlane(dir.x, leader), rlane(dir.y, leader), rlane(dir.z, leader));
				const float k0 = rlane(kx, leader), kend = rlane(ky, leader);
				// (pixels outside the buffer have left the kernel: position j of the chain lives in the j-th ACTIVE lane)
				const uint64_t here = __builtin_amdgcn_ballot_w64(true);
				const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t) (here >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) here, 0u));
				float mine;
				{
					const float k1 = k0 + step, delta = k1 - k0, low = step - delta;
					const uint32_t e = __float_as_uint(k0) >> 23;
					const float half_ulp = __uint_as_float((e > 24u ? e - 24u : 1u) << 23), klast = VR_FMA(63.0f, delta, k0);
					const bool fast = rfl((e > 24u && (__float_as_uint(klast) >> 23) == e && __builtin_fabsf(low) != half_ulp && delta > 0.0f) ? 1u : 0u) != 0u;
					if (fast) mine = VR_FMA((float) rank, delta, k0);
					else {
						float run = k0;
						mine = k0;
						#pragma nounroll
						for (uint32_t j = 1; j < 64u; j++) { run = run + step; mine = rank >= j ? run : mine; }
					}
				}
				const f3 lp = march_point<SAMPLING>(lo, ld, mine);
				const BlockIdx lb = block_index(a, lp);
				bool goes_on = mine <= kend && block_empty(lds, lb);
				if (goes_on) goes_on = leap_empty_space(a, lb, lp, ld) == 0.0f;
				const uint64_t stops = here & ~__builtin_amdgcn_ballot_w64(goes_on);
				const int first = stops != 0ull ? __builtin_ctzll(stops) : 63 - __builtin_clzll(here);      // the first position that does not go on (else the last: the step below re-evaluates it)
				const float k_new = rlane(mine, first);
				if ((int) lane == leader) { kx = k_new; pt = march_point<SAMPLING>(origin, dir, kx); }
				if (__builtin_popcountll(here & ((1ull << first) - 1ull)) < 4) coop_pause = 24;
			}
			bool zl = false;
			if (probing) {
				const BlockIdx blk = block_index(a, pt);
				if (kx <= ky && block_empty(lds, blk)) {
					const float leap = leap_empty_space(a, blk, pt, dir);
					zl = leap == 0.0f;
					kx += leap;
					kx += step;
					pt = march_point<SAMPLING>(origin, dir, kx);
				} else {
					probing = false;
				}
			}
			zero_leap = __builtin_amdgcn_ballot_w64(zl);
		}
	}
	alive = alive && (kx <= ky);                    // CPURenderer.cpp:26-27: fully empty ray — pixel keeps the clear value
	const bool visible = alive;

	// -- colour accumulation loop (CPURenderer.cpp:29-39 / GPURenderer4.cu:75-86), front to back, premultiplied
	f4 acc; acc.x = acc.y = acc.z = acc.w = 0.0f;
	const f3 light = ld3(a.p.view.light_pos);
	const float kd = a.p.light_kd;
	const bool lit = kd > 0.01f;
	const float threshold = a.p.ray_threshold;
	if (SAMPLING == VR_SAMPLE_NEAREST) {
		// Same loop shape as the TRILINEAR branch below (prefetch of sample i+1, finished lanes composited with weight 0,
		// per-wave transparent-sample shortcut, two samples per exit vote); the arithmetic is the reference's, unfused:
		// acc + cur * 0 == acc exactly, and map_float_int clamps every index, so speculative fetches stay in bounds.
		// In-bounds speculative fetches without clamping to 0: every fetch position is taken at min(k, ky), on the ray's own
		// segment inside the cube (for live lanes that IS the sample position); lanes without a segment march position 0.
		// clamp_fetch (far-away views, see TRILINEAR) falls back to the reference's two-sided clamp.
		const int tf_zero_idx = (int) a.tf_zero_below;                 // entries 0..tf_zero_idx are (0,0,0,0)
		const int opaque_above = (tf_zero_idx + 1) * VR_TF_RATIO * (BPV == 1 ? 1 : 256) - 1;
		uint64_t live = __builtin_amdgcn_ballot_w64(alive);            // liveness as one scalar wave mask (see TRILINEAR)
		if (!alive) { kx = 0.0f; ky = 0.0f; origin = mk3(0.0f, 0.0f, 0.0f); dir = origin; pt = origin; }
		constexpr bool kTables = is_brick_table_layout(LAYOUT) && ADDR != kAddrWide;  // padded address tables (kLutPad)
		auto march = [&](auto clamp_tag, auto scaled_tag) {
		constexpr bool kClamp = decltype(clamp_tag)::value;
		// kFree: fetch positions are NOT pulled back to the ray's segment — a finished lane's k simply stops (its step becomes 0, a
		// wave-uniform branch when a lane finishes), so a speculative position lies at most two steps past the exit point, inside
		// the table padding.  Otherwise (no tables, or the clamping variant) every fetch position is taken at min(k, ky) / clamped.
		constexpr bool kFree = !kClamp && kTables;
		constexpr bool kScaled = kFree && decltype(scaled_tag)::value;               // sample_nearest_scaled
		constexpr bool kLazy = kFree && VR_LAZY_EXIT;
		const f3 so = kScaled ? mk3(origin.x * a.half_x, origin.y * a.half_y, origin.z * a.half_z) : origin;
		const f3 sd = kScaled ? mk3(dir.x * a.half_x, dir.y * a.half_y, dir.z * a.half_z) : dir;
		float step_v = kFree ? select_lanes(live, step) : step;
		auto fetch_at = [&](float k) {
			if (!kClamp && !kFree) k = __builtin_fminf(k, ky);
			const f3 p = mk3(so.x + sd.x * k, so.y + sd.y * k, so.z + sd.z * k);      // CPURenderer.cpp:17,24,38: two roundings per axis
			if (kClamp) return sample_nearest<BPV, ADDR, LAYOUT, true>(vol, a, lut, p);
			if (kScaled) return sample_nearest_scaled<BPV, ADDR, LAYOUT, true>(vol, a, lut, p);
			return sample_nearest_incube<BPV, ADDR, LAYOUT, true>(vol, a, lut, p);
		};
		constexpr bool kManaged = Managed<BPV, ADDR, LAYOUT>::value;
		// kDepth samples ahead: slot j carries the fetched word and the k of its sample
		uint32_t word[kSlots]; float ks[kSlots];
		ks[0] = kx; word[kSlots - 1] = 0;
		static_for<0, kDepth>([&](auto j) {
			if constexpr (j.value > 0) ks[j.value] = ks[j.value - 1] + step_v;
			word[j.value] = fetch_at(ks[j.value]);
		});
		auto step_sample = [&](auto jc) {
			constexpr int c = decltype(jc)::value, n = (c + kDepth) % kSlots, nx = (c + 1) % kSlots;
			ks[n] = ks[(n + kSlots - 1) % kSlots] + step_v;
			word[n] = fetch_at(ks[n]);
			__builtin_amdgcn_sched_barrier(0);
			kx = ks[c];
			const float kn = ks[nx];
			(void) kn;
			// Nothing that reads the fetched word may move above this point: the compiler otherwise hoists such work to the loop latch,
			// behind an s_waitcnt vmcnt(0) that drains the prefetches in flight once per iteration.
			if (kManaged) { pin(word[c]); managed_wait<kDepth>(); pin(word[c]); }
			else pin(word[c]);
			const uint32_t s = voxel_of<BPV, LAYOUT>(word[c]);
			// transfer_fn[sample / TF_RATIO] (CPURenderer.cpp:31) is (0,0,0,0) for index <= tf_zero_idx, i.e. for
			// s <= opaque_above = (tf_zero_idx + 1) * TF_RATIO * (1 or 256) - 1: tested on the voxel itself, the index is only formed
			// by the few samples that get past the test
			if ((__builtin_amdgcn_sicmp((int) s, opaque_above, kIcmpSGT) & live) != 0ull && VR_OPEN_LANES(acc.w, live) != 0ull) {
				if (kLazy) {                                                                      // this sample's own segment test (see the loop)
					const uint64_t inside = __builtin_amdgcn_fcmpf(kx, ky, kFcmpOLE);
					if ((live & ~inside) != 0ull) { live &= inside; step_v = select_lanes(live, step); }       // a lane that is dropped here stops HERE:
				}                                                                                 // the rotation test only looks at lanes still marked live
				uint32_t idx = (BPV == 1 ? s : (s >> 8)) / VR_TF_RATIO;
				asm volatile("" : "+v"(idx));                                                       // keep the index arithmetic inside the branch
				f4 cur = lds.tf[idx];
				const uint64_t shaded = lit ? (__builtin_amdgcn_fcmpf(cur.w, 0.05f, kFcmpOGT) & live) : 0ull;
				if (shaded != 0ull) {                                                             // RaycasterBase.h:87-98 shade
					const float raw = BPV == 1 ? 255.0f : 65535.0f;
					pt = march_point<SAMPLING>(origin, dir, kx);                                  // the sample's own position
					f3 d = mk3(light.x - pt.x, light.y - pt.y, light.z - pt.z);
					float inv = 1.0f / __builtin_sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
					f3 l = mk3(d.x * inv, d.y * inv, d.z * inv);
					f3 ps = mk3(pt.x + l.x * 0.01f, pt.y + l.y * 0.01f, pt.z + l.z * 0.01f);
					const uint32_t s_l = voxel_of<BPV, LAYOUT>(sample_nearest<BPV, ADDR, LAYOUT>(vol, a, lut, ps));
					const float sl = BPV == 1 ? lds.unit[s_l] : (float) s_l / raw;                  // RaycasterBase.h:93-96
					const float sc = BPV == 1 ? lds.unit[s] : (float) s / raw;
					const float diffuse = select_lanes(shaded, (sl - sc) * kd);                   // x + 0 == x: unshaded lanes unchanged
					cur.x += diffuse; cur.y += diffuse; cur.z += diffuse;
				}
				const float t = select_lanes(live, 1 - acc.w);                                    // CPURenderer.cpp:34
				acc.x = acc.x + cur.x * t; acc.y = acc.y + cur.y * t;
				acc.z = acc.z + cur.z * t; acc.w = acc.w + cur.w * t;
				live &= ~__builtin_amdgcn_fcmpf(acc.w, threshold, kFcmpOGT);                      // CPURenderer.cpp:35-36
				if (kFree) step_v = select_lanes(live, step);                                     // terminated rays stop marching
			}
			if (!kLazy) {
				const uint64_t still = __builtin_amdgcn_fcmpf(kn, ky, kFcmpOLE);
				if (kFree && (live & ~still) != 0ull) step_v = select_lanes(live & still, step);      // a lane has just left its segment
				live &= still;
			}
		};
		// kLazy: `live` is brought up to date once per rotation of the slots (the k of the next sample against the end of the segment),
		// and by every sample that composites, for itself.  In between a finished lane still counts as live: its fetches lie in the
		// table padding (kOverrunSteps), a transparent sample does nothing with it, a compositing sample tests it first.
		while (live != 0ull) {
			static_for<0, kSlots>(step_sample);
			if (kLazy) {
				const uint64_t still = __builtin_amdgcn_fcmpf(ks[0], ky, kFcmpOLE);
				if ((live & ~still) != 0ull) step_v = select_lanes(live & still, step);
				live &= still;
			}
		}
		if (kManaged) {                                              // nothing in flight into registers we release
			static_for<0, kSlots>([&](auto j) { pin(word[j.value]); });
			managed_wait<0>();
			static_for<0, kSlots>([&](auto j) { pin(word[j.value]); });
		}
		};
		if (a.clamp_fetch) march(std::true_type(), std::false_type());
		else if (kTables && a.near_scaled) march(std::false_type(), std::true_type());
		else march(std::false_type(), std::false_type());
	} else {
		// texel-space ray: coordinate = fma(k, A, B) (see oracle/vr_oracle.c axis_setup)
		f3 A = mk3(dir.x * a.half_x, dir.y * a.half_y, dir.z * a.half_z);
		f3 B = mk3(VR_FMA(origin.x, a.half_x, a.off_x), VR_FMA(origin.y, a.half_y, a.off_y), VR_FMA(origin.z, a.half_z, a.off_z));
		// Lanes that are finished keep executing an in-bounds fetch with a zero weight instead of being masked off:
		// acc = fma(cur, 0, acc) leaves them bit-for-bit unchanged, and the loop body needs no per-lane control flow
		// except the shading block.  The wave leaves when no lane is alive.
		// In bounds without clamping three coordinates per sample: every fetch position is taken at min(k, ky), i.e. on the
		// ray's own segment inside the cube, where truncation alone gives the clamped cell (tri_issue); lanes that never
		// had a segment march the constant position 0.  The host switches the coordinate clamp back on (clamp_fetch) for
		// views so far from the volume that fp32 rounding of the coordinates could leave (-1, N).
		if (!alive) { kx = 0.0f; ky = 0.0f; A = mk3(0.0f, 0.0f, 0.0f); B = A; }
		// kLayoutRunDual, tile on the copy along y: the texel-space ray is kept with y and z EXCHANGED — that is what the tile's
		// address tables index (staging above); the few samples that are filtered put the two coordinates back (same fma, same bits)
		if (LAYOUT == kLayoutRunDual && group_sched[3] != 0u) { float t = A.y; A.y = A.z; A.z = t; t = B.y; B.y = B.z; B.z = t; }
		constexpr bool kTables = LAYOUT != kLayoutLinear && ADDR != kAddrWide;        // padded address tables (kLutPad)
		auto march = [&](auto clamp_tag) {                    // instantiated for both settings: no per-sample test of the flag
			constexpr bool kClamp = decltype(clamp_tag)::value;
			constexpr bool kFree = !kClamp && kTables;        // see the NEAREST loop: no min(k, ky), finished lanes stop instead
			constexpr bool kLazy = kFree && VR_LAZY_EXIT;     // exit test once per rotation of the slots (see the NEAREST loop)
			// Software pipeline: the loads of sample i+2 are issued before sample i is
			// unpacked, filtered and composited, so memory round trips overlap the arithmetic inside every wave (on top of the
			// 8 waves per SIMD).  The body is written once (`step_sample`) and instantiated once per fetch slot and iteration
			// with the slots rotated: no register copies, one exit vote per three samples (a finished wave at worst composites
			// two more weight-0 samples).
			auto issue = [&](float k) {
				if (!kClamp && !kFree) k = __builtin_fminf(k, ky);
				return tri_issue<BPV, ADDR, LAYOUT, true>(vol, a, lut, VR_FMA(k, A.x, B.x), VR_FMA(k, A.y, B.y), VR_FMA(k, A.z, B.z), kClamp);
			};
			constexpr bool kManaged = ManagedTri<BPV, ADDR, LAYOUT>::value;
			// Lane liveness is kept as ONE 64-bit wave mask in scalar registers (`live`), updated with v_cmp results
			// (__builtin_amdgcn_fcmpf returns the wave's compare mask) — no per-lane control flow, no mask <-> VGPR round trips:
			// the body is straight-line code with two wave-uniform branches (transparent shortcut, shading block).
			uint64_t live = __builtin_amdgcn_ballot_w64(alive);
			float step_v = kFree ? select_lanes(live, step) : step;       // per-lane step: 0 once the lane is finished
			// kDepth samples ahead (three for 2-byte voxels, whose slots hold four words: 64 VGPRs keep 8 waves per SIMD):
			// slot j carries the fetched words and the k of its sample
			// (the clipped linear-array kernels as well: a slot of theirs holds four words whatever the voxel size — their unclipped twins for 1-byte
			// voxels, not on any default path, take 72-74 VGPRs)
			constexpr bool kFourWordSlots = BPV == 2 || (CLIP && LAYOUT == kLayoutLinear);
			// (a shadowed frame: one sample less ahead — with the factor fetch of its dense block the full depth takes 66-69 VGPRs, 7 waves per SIMD;
			// a gradient-lit frame likewise: one or two gradient fetches are in flight inside its dense block; a slab frame likewise: the previous
			// sample's coordinate crosses the march and a wide slab holds two integrals beside the colour)
			constexpr int kFullDepth = is_run_layout(LAYOUT) ? kRunDepth : (!kFourWordSlots ? vr::kDepth : (vr::kDepth > kDepthTwoByte ? kDepthTwoByte : vr::kDepth));
			// (a backdrop frame likewise: its base family carries the shadow's factor fetch behind a kernel argument, the others are lit or slab frames)
			constexpr int kDepth = (SHADOW || LIT || SLAB || BACKDROP) && kFullDepth > 1 ? kFullDepth - 1 : kFullDepth, kSlots = kDepth + 1;
			TriFetch<BPV, LAYOUT> f[kSlots]; float ks[kSlots];
			ks[0] = kx;
			// SLAB: the clamped transfer-function coordinate of the previous sample of this loop; below 0 = there is none yet (the first
			// sample is every lane's first: ks[0] is the lane's own kx), and the sample's own coordinate stands in
			// kSlabLazy (shortcut variant (a), the default; VR_SLAB_LAZY=0 builds variant (b), which resolves every sample): shortcut (1)
			// stays — taken when the corners are low AND no live lane's previous coordinate is above tf_zero_below, for a slab that
			// ends in transparent values but starts in dense ones is not transparent — and a skipped sample leaves tp = -2: "not
			// resolved".  The first sample behind a run of skipped ones resolves its predecessor then, from a copy of that slot's words
			// and k taken before the prefetch re-issues the slot: the exact coordinate, at the price of the copy.
#ifndef VR_SLAB_LAZY
#define VR_SLAB_LAZY 1
#endif
			constexpr bool kSlabLazy = SLAB && VR_SLAB_LAZY;
			float tp = -1.0f;
			(void) tp;
			if constexpr (kSlabLazy) ks[kSlots - 1] = kx;                       // (read by the first sample's copy, never used)
			f[kSlots - 1].w0 = f[kSlots - 1].w1 = f[kSlots - 1].w2 = f[kSlots - 1].w3 = 0; f[kSlots - 1].q = 0; f[kSlots - 1].q2 = 0; f[kSlots - 1].o = (u32x4) (0u);
			static_for<0, kDepth>([&](auto j) {
				if constexpr (j.value > 0) ks[j.value] = ks[j.value - 1] + step_v;
				f[j.value] = issue(ks[j.value]);
			});
			auto step_sample = [&](auto jc) {
				constexpr int c = decltype(jc)::value, n = (c + kDepth) % kSlots, nx = (c + 1) % kSlots;
				TriFetch<BPV, LAYOUT> before = f[n];                                    // kSlabLazy: slot n held the previous sample
				const float k_before = ks[n];
				(void) before; (void) k_before;
				ks[n] = ks[(n + kSlots - 1) % kSlots] + step_v;
				f[n] = issue(ks[n]);
#ifndef VR_NO_SCHED_BARRIER
				__builtin_amdgcn_sched_barrier(0);
#endif
				TriFetch<BPV, LAYOUT> &cur = f[c];
				kx = ks[c];
				const float kn = ks[nx];
				(void) kn;
			(void) kn;
				// Exact shortcuts, decided per wave.  Entries 0..tf_zero_below of the premultiplied TF are all zero (the reference's
				// default TF is zero below 10 % density), so a sample whose TF coordinate tb is <= tf_zero_below has colour
				// (0,0,0,0), is never shaded (alpha 0 <= 0.05) and leaves acc bit-for-bit unchanged.
				//  (1) before any arithmetic: if all 8 corner voxels of every live lane are below the power of two `skip_below`
				//      (a bit test on the packed words), the interpolated value is too — a lerp never leaves [min, max] of its
				//      operands, fp32 rounding included — and skip_below was chosen on the host so that tb <= tf_zero_below
				//      follows: the wave skips unpacking, the 7 lerps and everything after them;
				//  (2) after the interpolation: the same test on tb itself skips the LDS lookups, the shading test and the composite.
				// pinned below the issue (see the NEAREST loop), on the slot's own registers: waits only for the slot's loads
				if (kManaged && is_run_layout(LAYOUT)) {               // one 8-byte gather per slot: kDepth younger ones may be in flight
					pin(cur.q); managed_wait<kDepth>(); pin(cur.q);
					cur.w0 = (uint32_t) cur.q; cur.w1 = (uint32_t) (cur.q >> 32);
				} else if (kManaged && LAYOUT == kLayoutOct) {         // one 16-byte gather per slot (2-byte voxels, oct bricks)
					pin(cur.o); managed_wait<kDepth>(); pin(cur.o);
					cur.w0 = cur.o.x; cur.w1 = cur.o.y; cur.w2 = cur.o.z; cur.w3 = cur.o.w;
				} else if (kManaged && BPV == 2) {                     // two 8-byte gathers per slot (2-byte voxels)
					pin(cur.q, cur.q2); managed_wait<2 * kDepth>(); pin(cur.q, cur.q2);
					cur.w0 = (uint32_t) cur.q; cur.w1 = (uint32_t) (cur.q >> 32); cur.w2 = (uint32_t) cur.q2; cur.w3 = (uint32_t) (cur.q2 >> 32);
				} else if (kManaged) {                                 // two 4-byte gathers per slot: 2 * kDepth younger ones
					pin(cur.w0, cur.w1); managed_wait<2 * kDepth>(); pin(cur.w0, cur.w1);
				} else if (LAYOUT != kLayoutLinear && BPV == 1) pin(cur.w0, cur.w1);
				else pin(cur.w0, cur.w1, cur.w2, cur.w3);
				const TriFetch<BPV, LAYOUT> &now = cur;
				uint32_t corners;
				if (LAYOUT != kLayoutLinear) corners = BPV == 1 ? (now.w0 | now.w1) : (now.w0 | now.w1 | now.w2 | now.w3);
				else                          corners = now.w0 | now.w1 | now.w2 | now.w3;
				// skip_cmp is 0; a TF without leading zero entries (nothing may be skipped) comes with skip_mask 0 and skip_cmp 1: 0 != 1 always
				// SLAB: the next sample needs this one's coordinate exactly, transparent or not.  Variant (b) resolves every sample; variant (a),
				// kSlabLazy above, keeps shortcut (1) and resolves a skipped sample when its successor asks.  (2) is widened to "this
				// coordinate and the previous one" (K is exactly 0 up to tf_zero_below).  The saturation shortcut stays: a lane whose alpha
				// is exactly 1 composites with weight 0 for good, whatever its tp is by then.
				if (((SLAB && !kSlabLazy) ||
				     ((kSlabLazy ? (__builtin_amdgcn_uicmp(corners & a.skip_mask, a.skip_cmp, kIcmpNE) | __builtin_amdgcn_fcmpf(tp, a.tf_zero_below, kFcmpOGT))
				                 : __builtin_amdgcn_uicmp(corners & a.skip_mask, a.skip_cmp, kIcmpNE)) & live) != 0ull) && VR_OPEN_LANES(acc.w, live) != 0ull) {
				if (kLazy) {
					const uint64_t inside = __builtin_amdgcn_fcmpf(kx, ky, kFcmpOLE);
					if ((live & ~inside) != 0ull) { live &= inside; step_v = select_lanes(live, step); }
				}
				const float xb = VR_FMA(kx, A.x, B.x);                                                            // where the words were fetched
				float yb = VR_FMA(kx, A.y, B.y), zb = VR_FMA(kx, A.z, B.z);
				// kLayoutRunDual: read again from LDS here, so that the flag occupies no register across the march — through an index the
				// compiler cannot see through, or it hoists the read out of the loop (a volatile access would become a FLAT load with a
				// vmcnt(0) wait behind it: the whole prefetch pipeline drained per filtered sample)
				bool along_y = false;
				if (LAYOUT == kLayoutRunDual) {
					uint32_t opaque_zero;
					asm volatile("v_mov_b32 %0, 0" : "=v"(opaque_zero));
					along_y = group_sched[3u + opaque_zero] != 0u;
				}
				if (LAYOUT == kLayoutRunDual && along_y) { const float t = yb; yb = zb; zb = t; }                 // the true coordinates again
				const float raw = tri_resolve<BPV, LAYOUT, kQ8>(now, a, xb, yb, zb, along_y);                 // GPURenderer4.cu:76
				// GPURenderer4.cu:77 filtered TF: texel coordinate tb, entries floor(tb) and floor(tb)+1
				const float tb = __builtin_amdgcn_fmed3f(VR_FMA(raw, a.tf_scale, -0.5f), 0.0f, (float) (VR_TF_SIZE - 1));
				if constexpr (kSlabLazy) {
					if (__builtin_amdgcn_ballot_w64(tp == -2.0f) != 0ull) {                                       // wave-uniform: the previous sample was skipped
						const float raw_p = tri_resolve<BPV, LAYOUT, kQ8>(before, a, VR_FMA(k_before, A.x, B.x), VR_FMA(k_before, A.y, B.y), VR_FMA(k_before, A.z, B.z));
						tp = __builtin_amdgcn_fmed3f(VR_FMA(raw_p, a.tf_scale, -0.5f), 0.0f, (float) (VR_TF_SIZE - 1));
					}
				}
				const float tq = SLAB ? (tp < 0.0f ? tb : tp) : tb;                                              // SLAB: the front of the slab
				if constexpr (SLAB) tp = tb;
				if (((SLAB ? (__builtin_amdgcn_fcmpf(tb, a.tf_zero_below, kFcmpOGE) | __builtin_amdgcn_fcmpf(tq, a.tf_zero_below, kFcmpOGE))
				           : __builtin_amdgcn_fcmpf(tb, a.tf_zero_below, kFcmpOGE)) & live) != 0ull) {
					f4 c;
					{
						const float tm = SLAB ? 0.5f * (tq + tb) : tb;                                             // a narrow slab: the lookup at its middle (tb itself where d is 0)
						const uint32_t i = (uint32_t) (int) tm;
						const float w = filter_weight<kQ8>(__builtin_amdgcn_fractf(tm));
						const f4 c0 = lds.tf[i], dc = lds.dtf[i];
						c.x = VR_FMA(w, dc.x, c0.x); c.y = VR_FMA(w, dc.y, c0.y);
						c.z = VR_FMA(w, dc.z, c0.z); c.w = VR_FMA(w, dc.w, c0.w);
					}
					if constexpr (SLAB) {
						// a wide slab, |d| >= 0.5: c = (K(tb) - K(tp)) / d, the mean of the transfer function over the slab, with full fp32 weights in
						// both sampling modes; the division, the difference and the product each rounded once (include/vr_hip.h)
						const float d = tb - tq;
						const uint64_t wide = __builtin_amdgcn_fcmpf(__builtin_fabsf(d), 0.5f, kFcmpOGE) & live;
						if (wide != 0ull) {
							auto integral = [&](float t) {
								const uint32_t i0 = (uint32_t) t, i = i0 < (uint32_t) (VR_TF_SIZE - 2) ? i0 : (uint32_t) (VR_TF_SIZE - 2);
								const float w = t - (float) i, hw = 0.5f * w;
								const f4 c0 = lds.tf[i], dc = lds.dtf[i], k0 = slab_k[i];
								f4 r;
								r.x = VR_FMA(w, VR_FMA(hw, dc.x, c0.x), k0.x); r.y = VR_FMA(w, VR_FMA(hw, dc.y, c0.y), k0.y);
								r.z = VR_FMA(w, VR_FMA(hw, dc.z, c0.z), k0.z); r.w = VR_FMA(w, VR_FMA(hw, dc.w, c0.w), k0.w);
								return r;
							};
							// (register diet: the front's integral is complete before the back's three table reads are issued)
							f4 kp = integral(tq);
							asm volatile("" : "+v"(kp.x), "+v"(kp.y), "+v"(kp.z), "+v"(kp.w));
							__builtin_amdgcn_sched_barrier(0);
							const f4 kb = integral(tb);
							const float r = 1.0f / d;
							c.x = select_lanes_else(wide, (kb.x - kp.x) * r, c.x); c.y = select_lanes_else(wide, (kb.y - kp.y) * r, c.y);
							c.z = select_lanes_else(wide, (kb.z - kp.z) * r, c.z); c.w = select_lanes_else(wide, (kb.w - kp.w) * r, c.w);
						}
					}
					if constexpr (!LIT) {
						const uint64_t shaded = lit ? (__builtin_amdgcn_fcmpf(c.w, 0.05f, kFcmpOGT) & live) : 0ull;   // GPURenderer4.cu:78
						if (shaded != 0ull) {                                                              // GPURenderer4.cu:41-51 shade_texture
							const f3 p3 = march_point<SAMPLING>(origin, dir, kx);
							const f3 d = mk3(light.x - p3.x, light.y - p3.y, light.z - p3.z);
							const float inv = rsqrt_nr(VR_FMA(d.z, d.z, VR_FMA(d.y, d.y, d.x * d.x)));
							const float lx = VR_FMA(d.x * inv, a.lh_x, xb), ly = VR_FMA(d.y * inv, a.lh_y, yb), lz = VR_FMA(d.z * inv, a.lh_z, zb);
							TriFetch<BPV, LAYOUT> lf;
							if (LAYOUT == kLayoutRunDual) {                     // clamp with the true bounds, then hand the tile's table order over
								const float cy = __builtin_amdgcn_fmed3f(ly, 0.0f, a.max_y), cz = __builtin_amdgcn_fmed3f(lz, 0.0f, a.max_z);
								lf = tri_issue<BPV, ADDR, LAYOUT>(vol, a, lut, __builtin_amdgcn_fmed3f(lx, 0.0f, a.max_x), along_y ? cz : cy, along_y ? cy : cz, false);
							} else lf = tri_issue<BPV, ADDR, LAYOUT>(vol, a, lut, lx, ly, lz, true);
							const float raw_l = tri_resolve<BPV, LAYOUT, kQ8>(lf, a, lx, ly, lz, along_y);
							const float diffuse = select_lanes(shaded, (raw_l - raw) * a.kd_scaled);       // 0 for lanes that are not shaded
							c.x += diffuse; c.y += diffuse; c.z += diffuse;
						}
					}
					if constexpr (LIT) {                                                               // vr_hip_set_lighting: the cue above gives way to Blinn-Phong from the field's gradient
						const uint64_t dense = __builtin_amdgcn_fcmpf(c.w, 0.05f, kFcmpOGT) & live;
						if (dense != 0ull) {
							// (register diet: only c.w and tb cross the gradient fetches — the colour is looked up again behind them, the same bits)
							float m, spec, tb2 = tb;
							light_sample<BPV, ADDR, LAYOUT, kQ8>(vol, a, lut, A, B, origin, dir, kx, dense, c.w, m, spec);
							if constexpr (SLAB) {                                                      // a slab's colour is not one lookup: it crosses the gradient fetches
								c.x = VR_FMA(c.x, m, spec); c.y = VR_FMA(c.y, m, spec); c.z = VR_FMA(c.z, m, spec);
							} else {
							asm volatile("" : "+v"(tb2));
							const uint32_t i2 = (uint32_t) (int) tb2;
							const float w2 = filter_weight<kQ8>(__builtin_amdgcn_fractf(tb2));
							const f4 c0 = lds.tf[i2], dc = lds.dtf[i2];
							c.x = VR_FMA(VR_FMA(w2, dc.x, c0.x), m, spec); c.y = VR_FMA(VR_FMA(w2, dc.y, c0.y), m, spec); c.z = VR_FMA(VR_FMA(w2, dc.z, c0.z), m, spec);
							}
							if (lit_frame_shadowed()) {                                                    // wave-uniform: a kernel argument (vr_hip_set_shadow composes)
								const float f = select_lanes_else(dense, shadow_factor(march_point<SAMPLING>(origin, dir, kx)), 1.0f);
								c.x *= f; c.y *= f; c.z *= f;
							}
						}
					}
					if constexpr ((SLAB || BACKDROP) && !LIT) {                                        // a slab frame and a backdrop frame take the shadow as composite_lit does: a kernel argument, wave-uniform
						if (lit_frame_shadowed()) {
							const uint64_t dense = __builtin_amdgcn_fcmpf(c.w, 0.05f, kFcmpOGT) & live;
							if (dense != 0ull) {
								const float f = select_lanes_else(dense, shadow_factor(march_point<SAMPLING>(origin, dir, kx)), 1.0f);
								c.x *= f; c.y *= f; c.z *= f;
							}
						}
					}
					if constexpr (SHADOW) {                                                            // vr_hip_set_shadow: dense samples are scaled by the light grid, lit or not
						const uint64_t dense = __builtin_amdgcn_fcmpf(c.w, 0.05f, kFcmpOGT) & live;
						if (dense != 0ull) {
							const float f = select_lanes_else(dense, shadow_factor(march_point<SAMPLING>(origin, dir, kx)), 1.0f);      // x * 1 == x: other lanes unchanged
							c.x *= f; c.y *= f; c.z *= f;
						}
					}
					const float t = select_lanes(live, 1 - acc.w);                                     // finished lanes: weight 0
					acc.x = VR_FMA(c.x, t, acc.x); acc.y = VR_FMA(c.y, t, acc.y);
					acc.z = VR_FMA(c.z, t, acc.z); acc.w = VR_FMA(c.w, t, acc.w);
					live &= ~__builtin_amdgcn_fcmpf(acc.w, threshold, kFcmpOGT);                        // ERT (CPURenderer.cpp:35-36)
					if (kFree) step_v = select_lanes(live, step);                                       // terminated rays stop marching
				}
				} else if constexpr (kSlabLazy) tp = -2.0f;                                                 // skipped: resolved later, if a sample needs it
				if (!kLazy) {
					const uint64_t still = __builtin_amdgcn_fcmpf(kn, ky, kFcmpOLE);                    // the loop condition
					if (kFree && (live & ~still) != 0ull) step_v = select_lanes(live & still, step);    // a lane has just left its segment
					live &= still;
				}
			};
			while (live != 0ull) {
				static_for<0, kSlots>(step_sample);
				if (kLazy) {
					const uint64_t still = __builtin_amdgcn_fcmpf(ks[0], ky, kFcmpOLE);
					if ((live & ~still) != 0ull) step_v = select_lanes(live & still, step);
					live &= still;
				}
			}
			if (kManaged) {                                            // nothing in flight into registers we release
				auto pin_slot = [&](auto j) { if (is_run_layout(LAYOUT)) pin(f[j.value].q); else if (LAYOUT == kLayoutOct) pin(f[j.value].o); else if (BPV == 2) pin(f[j.value].q, f[j.value].q2); else pin(f[j.value].w0, f[j.value].w1); };
				static_for<0, kSlots>(pin_slot);
				managed_wait<0>();
				static_for<0, kSlots>(pin_slot);
			}
		};
		if (a.clamp_fetch) march(std::true_type()); else march(std::false_type());
	}

	// -- RaycasterBase.h:44-50 write_color (+ the fused clear: misses and fully-empty rays store 0)
	uint32_t rgba = 0;
	if (hit && visible) {
		rgba = map_float_int(acc.x, 256) | (map_float_int(acc.y, 256) << 8) |
		       (map_float_int(acc.z, 256) << 16) | (map_float_int(acc.w, 256) << 24);
	}
	if constexpr (BACKDROP) {
		// a pixel with a surface: the layer's colour word bit for bit where nothing was composited, else the accumulated colour over it
		const size_t px = pixel;
		out_px = backdrop_out_at(px);
		if (backdrop_depth_at(px) >= 0.0f) {
			const uint32_t b = backdrop_rgba_at(px);
			if (hit && visible) {
				const float t = 1.0f - acc.w;
				auto over = [&](uint32_t byte, float c) { return map_float_int(VR_FMA(((float) byte + 0.5f) * (1.0f / 256.0f), t, c), 256); };
				rgba = over(b & 0xffu, acc.x) | (over((b >> 8) & 0xffu, acc.y) << 8) | (over((b >> 16) & 0xffu, acc.z) << 16) | (over(b >> 24, acc.w) << 24);
			} else rgba = b;
		}
	}
	*out_px = rgba;
	// cost of the tile = the end of its last wave after the start of the workgroup, in 64-cycle units (at least 1); every wave
	// reports, through the first of its lanes that is still here
	const uint32_t lane_id = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
	if (lane_id == (uint32_t) __builtin_ctzll(__builtin_amdgcn_ballot_w64(true))) {
		const uint32_t *w = group_sched;
		const uint64_t slot = ((uint64_t) w[2] << 32) | w[1];
		if (slot != 0ull) atomicMax((uint32_t *) (uintptr_t) slot, ((uint32_t) (__builtin_readcyclecounter() >> 6) - w[0]) | 1u);
	}
