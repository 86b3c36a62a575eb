/* das_staged.hip -- row-column DAS with the RF staged in LDS (gfx950 / MI355X): the headline kernel.
 *
 * Same arithmetic contract and the same delay factorisation as das_separable.hip
 * (idx = T(a; v_tx, z) + R(c; v_rx, z), shaders/das.glsl:204-231 of the reference), for
 * linear interpolation of complex samples -- the configuration the headline metric runs.
 *
 * das_separable.hip gathers 16 bytes per (voxel, channel, transmit) term straight from global
 * memory and sits on the CU's vector-memory path: 16.3 clk per wave64 gather instruction
 * (tools/microbench.hip).  But the 1024 voxels of a 32 x 32 tile touch only a short window of
 * every RF row: the receive delay moves by at most pitch*fs/c (0.6 sample at config 4) per voxel
 * along the receive axis and less along the transmit axis.  So per channel the block copies,
 * for every transmit, one W-sample window (W = 32 or 64) of the RF row into LDS -- 19 KB of
 * coalesced loads per channel instead of 1.2 MB of gathers through L1 -- and every lane then
 * interpolates out of LDS.
 *
 * Round 1's version of this kernel lost to the gather kernel (1327 against 1165 ms) because it
 * paid ~20 VALU instructions per term against the gather kernel's 14 (integer window bookkeeping,
 * an always-on range test, address arithmetic per tap), and VALU issue is what both kernels wait
 * for.  This version pays 9 (36 per batch of 4 terms):
 *   * the window position is folded into the FLOAT tables: element j of window (c, a) holds sample
 *     floor(rmin_c) + floor(tmin_a) + j (rmin / tmin: the delay minima over the tile); the receive
 *     table hands the lane R' = R - floor(rmin_c), the transmit table holds
 *     T'' = T - floor(tmin_a) - 1/2 -- all exact in f32 -- so ONE add gives the position p in the
 *     window, less 1/2.  (A sum of two small numbers is rounded at 2^-19 of a sample instead of the
 *     absolute index's 2^-12: closer to exact arithmetic than the shader it restates.)
 *   * window elements are LINES in window coordinates, {c_j, d_j} with d_j = s_(j+1) - s_j and
 *     c_j = s_j + (1/2 - j) d_j, 16 bytes: the two taps are ONE aligned ds_read_b128 and the
 *     interpolation ONE packed fma of the position itself, c_j + p d_j -- no fraction is formed;
 *   * no v_fract, no v_cvt: adding M = 2^23 + 2 + a*W rounds p to the nearest integer and leaves the
 *     window ELEMENT INDEX in the low mantissa bits of y = p + M (a packed add over two terms); the
 *     tap's LDS address is (bits(y) & 0xFFF) * 16, one v_lshlrev_b16 by 4 (full rate; a 16-bit op leaves the
 *     upper half of its result zero on gfx950, which drops M's exponent bits), because the staging area
 *     starts two elements into an LDS that holds nothing static and A4 * W <= 4096 elements;
 *   * transmits in pairs: one ds_read2_b64 serves four terms' delays, one ds_read_b128 two terms'
 *     phasors; the transmit table is padded to a multiple of 4 with zero phasors over a zero window
 *     row, so the last batch needs no select;
 *   * the range test of sample_rf (0 <= index < S - 1) is decided per lane and channel when the
 *     receive table is built (tile-wide extremes of T, as in das_separable.hip) and kept in the sign
 *     of the entry's weight; only waves with such a lane run the checked loop (absolute tap = window
 *     tap + the two floors; invalid taps read a zero element).
 *
 * Pipeline per channel: the buffer loads of the NEXT channel's windows are issued into registers
 * before the current channel is consumed and written to LDS after it (barrier - ds_write -
 * barrier); two 1024-thread blocks share a CU, so one block's barriers hide under the other's
 * arithmetic.  The host only launches this kernel when its bound on the delay spread of a tile fits
 * the window (plan_staged, executor.cpp).  No MFMA: gather-accumulate.  Measured (config 4, one
 * MI355X): 785-850 ms per 512^3 frame against 1116-1191 ms for the gather kernel; VALU 94 % busy,
 * 0.83-0.86 of the rate of its own VALU stream run without memory instructions.
 */
#include "das_staged_shared.h"

/* LDS (A4 = transmits rounded up to a multiple of 4; transmits are kept in PAIRS so that one read serves two terms):
 *   stage[a*W + j]   = { c_j, d_j }: the line through samples j and j + 1 of window (c, a) in window coordinates
 *                      (d_j = s' - s, c_j = s + (1/2 - j) d_j; s = sample floor(rmin_c) + floor(tmin_a) + j of row (c, a),
 *                      s' the next one); j < W, a < A4; two unused elements in front, one zero element behind   f32x4
 *   Tcs[(a/2)*V + v] = { cos(phi_t), sin(phi_t) of transmit a & ~1, then of transmit a | 1 }                   f32x4
 *   R[cl*U + u]      = { R' = r_index - floor(rmin_c), apod*cos(phi_r), apod*sin(phi_r), +-apod }   cl: channel in chunk;
 *                      the weight's sign bit set = the lane may leave the RF row (checked loop)                  f32x4
 *   Tz[(a/2)*V + v]  = { T'' = t_index - floor(tmin_a) - 1/2 of transmit a & ~1, of transmit a | 1 }             f32x2
 *   tfl[a]           = floor(tmin_a)  (checked loop and staging only),  rfloor[cl] = floor(rmin_c)               int */
/* NL: window elements a thread stages per channel, ceil(A4 * W / threads)
 * UNI: the tile is 64 voxels along the receive axis (= x), so a wave's lanes share ONE row of the transmit axis: the transmit
 *      delays and phasors are wave uniform.  They then come from a table in global memory (staged_tables_kernel below writes it
 *      once per frame, the same arithmetic the block otherwise does per tile) through SCALAR loads and enter the packed
 *      instructions as scalar operands: the LDS serves the four taps of a batch and nothing else (tools/microbench.hip
 *      loop_probe_uniform: 40.2 clk per term against 43.7, at a higher sustained clock). */
typedef __attribute__((address_space(4))) const f32x4 const_f32x4;
template <bool CW, int VS, int WS, int NL, bool UNI>
__device__ __forceinline__ void staged_body(const BfDasArgs &p, const BfSeparableArgs &q)
{
	extern __shared__ __attribute__((aligned(16))) f32x4 staged_lds[];
	/* WS: log2 of the window length (5, 6) */
	constexpr uint32_t V = 1u << VS, W = 1u << WS;
	const uint32_t U = 1u << q.u_shift;
	const int C = p.channel_count, A = p.acquisition_count, S = p.sample_count;
	const int A4 = (A + 3) & ~3;
	const int chunk = (int)q.channel_chunk;
	/* the staging area comes first and the kernel has no static LDS: 16 x (a window element's index + 2) IS its LDS
	 * address, which the inner loop forms with one shift */
	f32x4 *stage  = staged_lds + 2;                          /* (two unused elements in front: see the rounding of the inner loop) */
	f32x4 *Tcs    = stage + (size_t)A4 * W + 1;
	const size_t table_rows = UNI ? 0 : (size_t)(A4 / 2) * V;  /* (UNI: no transmit tables in LDS) */
	f32x4 *R      = Tcs + table_rows;
	f32x2 *Tz     = reinterpret_cast<f32x2 *>(R + (size_t)chunk * U);
	int   *tfl    = reinterpret_cast<int *>(Tz + table_rows);
	int   *rfloor = tfl + A4;
	f32x2 *wave_range = reinterpret_cast<f32x2 *>(rfloor + ((chunk + 1) & ~1));      /* 16 entries, 8-byte aligned */
	const uint32_t stage_elements = (uint32_t)A4 * W;

	uint32_t tu, tv, zl;
	if (!staged_tile_of(q, UNI, tu, tv, zl)) return;        /* whole block */
	const uint32_t z  = p.z_first + zl;

	const uint32_t u_axis = q.u_axis, v_axis = 1u - q.u_axis;
	const bool  rx_rows = (p.transmits[0].flags & BF_RX_ROWS) != 0;
	const uint32_t tid = threadIdx.x, nthreads = blockDim.x;
	if (q.depth_major & 2u) staged_violation_clear(tid);       /* STAGED_CHECKED: das_common.h */

	/* UNI: the tile's slice of the global table: [A4] floors, {lo, hi} of the absolute delays, then per lateral row of the tile and
	 * batch of 4 transmits 48 bytes: {T'' x 4}, {cos, sin} x 4 */
	const unsigned char *tile_tab = UNI ? reinterpret_cast<const unsigned char *>(q.tables) + (size_t)(zl * q.tiles[1] + tv) * q.table_stride : nullptr;
	f32x2 range;
	if constexpr (UNI) {
		for (uint32_t a = tid; a < (uint32_t)A4; a += nthreads) tfl[a] = reinterpret_cast<const int *>(tile_tab)[a];
		if (tid == 0) stage[stage_elements] = f32x4{0.f, 0.f, 0.f, 0.f};
		range = staged_uniform_range(*reinterpret_cast<const f32x2 *>(tile_tab + 4u * (uint32_t)A4));
	} else {
		staged_transmit_entries<VS, true>(p, v_axis, tv, z, tid, nthreads, [&](uint32_t a, uint32_t iv, uint32_t, float t_idx, float cs_c, float cs_s) {
			const uint32_t pair = (a >> 1) * V + iv, half = a & 1u;
			reinterpret_cast<f32x2 *>(Tcs + pair)[half] = f32x2{cs_c, cs_s};
			reinterpret_cast<float *>(Tz + pair)[half]  = t_idx;
		});
		if (tid == 0) stage[stage_elements] = f32x4{0.f, 0.f, 0.f, 0.f};
		range = rca_tile_range((uint32_t)A * V, wave_range, [&](uint32_t e) {
			uint32_t a = e >> VS, iv = e & (V - 1);
			return reinterpret_cast<const float *>(Tz + (a >> 1) * V + iv)[a & 1u];
		});
		for (uint32_t a = tid; a < (uint32_t)A4; a += nthreads)
			tfl[a] = staged_window_row<V, 2, 0>(reinterpret_cast<float *>(Tz + (size_t)(a >> 1) * V) + (a & 1u));
	}
	__syncthreads();                                         /* the floors are read below */

	/* the lane's voxel: needed for `inside` here and for the store at the very end -- recomputed there rather than held in two
	 * vector registers across the channel loop (the NL = 4 instances had none to spare) */
	uint32_t lu;
	bool inside;
	{
		uint32_t x0, y0, lv_unused;
		rca_voxel_of(tid, u_axis, U, q.u_shift, V, VS, tu, tv, x0, y0, lu, lv_unused);
		inside = x0 < p.size[0] && y0 < p.size[1];
	}

	f32x2 coherent   = {0.f, 0.f};
	float incoherent = 0.f;
	const f32x4   *Rl = R + lu;
	const uint32_t ulast = (uint32_t)(S - 1);
	/* LDS byte addresses */
	uint32_t tcs_base = (uint32_t)(uintptr_t)(lds_f32x4 *)Tcs;
	uint32_t tz_base  = (uint32_t)(uintptr_t)(lds_f32x2 *)Tz;
	/* opaque to the compiler: otherwise the static LDS in front of the dynamic block is re-added as a constant
	 * to every address of the inner loop instead of once here */
	asm("" : "+s"(tcs_base), "+s"(tz_base));

	/* staging (das_staged_shared.h): 8-byte samples, windows that start at the two floors */
	const __amdgpu_buffer_rsrc_t rf_rsrc = staged_rf_resource<f32x2>(p);
	uint32_t stage_inv[NL];
	staged_stage_offsets<f32x2, WS, 0>(stage_inv, tfl, A, S, tid, nthreads);
	auto stage_load = [&](int channel, int rfl, f32x2 (&regs)[NL]) { staged_stage_load(rf_rsrc, stage_inv, channel, A, S, rfl, regs); };
	/* Element j keeps the LINE through samples j and j + 1 in window coordinates, {c_j, d_j} with d_j = s_(j+1) - s_j and
	 * c_j = s_j + (1/2 - j) d_j, so that the interpolated sample at position p (measured from half a sample into the window,
	 * as the tables hold it) is c_j + p d_j for j = round(p): one packed fma of the position itself, no fraction needed.
	 * (At an integer position both neighbouring lines give the same value, so the tie of the rounding is harmless.)  The next
	 * sample sits in the next lane (a wave stages whole windows, consecutive lanes consecutive samples), fetched with a
	 * one-lane wave shift.  The last element of a window gets a meaningless line and is never selected (the host's window
	 * bound, plan_staged). */
	const float half_minus_j = 0.5f - (float)(tid & (W - 1));
	auto stage_store = [&](const f32x2 (&regs)[NL]) {
		#pragma unroll
		for (int n = 0; n < NL; n++) {
			const float sx = regs[n].x, sy = regs[n].y;
			const float nx = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, sx), 0x130, 0xf, 0xf, true));
			const float ny = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, sy), 0x130, 0xf, 0xf, true));
			const float dx = nx - sx, dy = ny - sy;
			const uint32_t e = tid + (uint32_t)n * nthreads;
			if (e < stage_elements) stage[e] = f32x4{__builtin_fmaf(half_minus_j, dx, sx), __builtin_fmaf(half_minus_j, dy, sy), dx, dy};
		}
	};

	for (int c0 = 0; c0 < C; c0 += chunk) {
		const int cn = (C - c0) < chunk ? (C - c0) : chunk;
		__syncthreads();        /* readers of the previous chunk's R / stage are done; the transmit tables are complete */
		staged_receive_table<f32x4, 0>(R, rfloor, c0, cn, tu, z, u_axis, q.u_shift, rx_rows, range, S, tid, nthreads);

		f32x2 regs[NL];
		stage_load(c0, rfloor[0], regs);
		for (int cl = 0; cl < cn; cl++) {
			__syncthreads();                   /* everyone is done with the previous channel's windows */
			stage_store(regs);
			__syncthreads();
			if (cl + 1 < cn) stage_load(c0 + cl + 1, rfloor[cl + 1], regs);   /* in flight during the arithmetic */
			if (!inside) continue;

			/* (register budget: 64 per lane at 8 waves per SIMD with the next channel's windows in flight.  The
			 * receive entry is read twice -- delay and aperture test here, phasor and weight after the loop -- and the
			 * lane's table addresses are rebuilt per channel rather than kept) */
			float r_rel, r_w;
			{
				const f32x4 r = Rl[(size_t)cl * U];
				r_rel = r.x; r_w = r.w;
			}
			if (__builtin_amdgcn_ballot_w64(r_w != 0.f) == 0) continue;    /* F# culling per wave */
			const bool wave_safe = !(q.depth_major & 2u) && __builtin_amdgcn_ballot_w64(__builtin_signbitf(r_w)) == 0;   /* bit 1: test hook, checked loop everywhere */
			f32x2 acc1 = {0.f, 0.f}, acc2 = {0.f, 0.f};
			f32x2 mag2 = {0.f, 0.f};
			/* one term: pos = position in the window (minus 1/2), tap = the line {c, d} of the element round(pos) selects */
			auto term = [&](f32x2 cs, float pos, f32x4 tap) -> float {
				f32x2 sv = f32x2{tap.x, tap.y} + pos * f32x2{tap.z, tap.w};
				acc1 += sv.x * cs;
				acc2 += sv.y * cs;
				if constexpr (CW) return hw_sqrt(__builtin_fmaf(sv.y, sv.y, sv.x * sv.x));
				else return 0.f;
			};
			auto batches = [&](auto checked) {
				constexpr bool CHECK = decltype(checked)::value;
				uint32_t lane_id = tid;
				asm volatile("" : "+v"(lane_id));                          /* not hoisted: see the register budget above */
				const uint32_t lane_v = u_axis == 0 ? lane_id >> q.u_shift : lane_id & (V - 1);
				uint32_t tcs_at = tcs_base + (lane_v << 4), tz_at = tz_base + (lane_v << 3);
				/* Position -> tap without v_fract / v_cvt / a fraction: adding M = 2^23 + 2 + (first window element of the batch)
				 * rounds the position to the nearest integer and leaves the ELEMENT INDEX 2 + a*W + round(p) in the low mantissa
				 * bits of y = p + M (packed: two terms per instruction); the tap's LDS byte address is (bits(y) & 0xFFF) * 16 --
				 * one 16-bit shift (full rate where 32-bit shifts and 24-bit multiplies are half rate; the upper half of a 16-bit
				 * result is zero on gfx950, so M's exponent bits drop out), no add: M's own bit pattern (0x4B000002 + a*W) contributes
				 * exactly 2 + a*W to the mantissa, a batch's base element 2 + a*W + round(p) is below 4096 (plan_staged: A4 * W <= 4096;
				 * rows 1-3 of the batch ride in the read's immediate offset), and the staging area starts two elements into an LDS
				 * that holds nothing static.  M is a scalar, stepped by 4*W
				 * per batch as an integer (the mantissa of a float in [2^23, 2^24) counts integers); term k's row k*W is the read's
				 * immediate offset.  The element is a line in window coordinates, so the interpolation uses p itself.
				 * Why 2^23 + 2: (1) p = -1/2 (the lane with the smallest delays of the tile) must round inside [2^23, 2^24) --
				 * just below 2^23 floats step by 1/2 and 2^23 - 1/2 would come back exact, with garbage in the low mantissa bits;
				 * (2) that tie must not round DOWN to the element in front of the row: 2 + a*W is even, so round-to-even takes it
				 * up to element 0.  At every other tie both neighbouring lines give the same value.
				 * (Tried and measured no faster: y = fma(p, 2^-149, B) into a denormal whose bit pattern is the index, then a
				 * 32-bit shift -- itself half rate, as it turned out -- instead of the 24-bit multiply: 0.721 of the gather kernel's
				 * time against 0.710.  The multiply before the 16-bit shift: 0.701 against 0.700.) */
				uint32_t m_bits = 0x4B000002u;
				[[maybe_unused]] bool window_left = false;    /* range-checked loop: some term selected an element outside its window */
				const f32x2 rr = {r_rel, r_rel};
				/* UNI: the wave's row of the global table (lv = tid >> 6 for a 64-wide tile), read through the constant address
				 * space so that the uniform reads become s_load_dwordx8 + s_load_dwordx4 per batch */
				const_f32x4 *uni_row = nullptr;
				if constexpr (UNI)
					uni_row = (const_f32x4 *)(uintptr_t)(tile_tab + 4u * (uint32_t)A4 + 16u +
					                                      (size_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)) * (size_t)(A4 / 4) * 48u);
				for (int a = 0; a < A4; a += 4, m_bits += 4u * W) {
					uint32_t at[4]; f32x4 tap[4];
					const float M = __builtin_bit_cast(float, m_bits);
					const f32x2 M2 = {M, M};
					f32x4 cs01, cs23; f32x2 tz01, tz23;
					if constexpr (UNI) {
						const f32x4 tz = uni_row[0];
						cs01 = uni_row[1]; cs23 = uni_row[2];
						tz01 = f32x2{tz.x, tz.y}; tz23 = f32x2{tz.z, tz.w};
						uni_row += 3;
					} else {
						cs01 = *(lds_f32x4 *)(uintptr_t)tcs_at;
						cs23 = *(lds_f32x4 *)(uintptr_t)(tcs_at + V * 16u);
						tz01 = *(lds_f32x2 *)(uintptr_t)tz_at;
						tz23 = *(lds_f32x2 *)(uintptr_t)(tz_at + V * 8u);
						tcs_at += 2u * V * 16u; tz_at += 2u * V * 8u;
					}
					const f32x2 p01 = rr + tz01, p23 = rr + tz23;
					const f32x2 y01 = p01 + M2,  y23 = p23 + M2;
					const float ys[4] = {y01.x, y01.y, y23.x, y23.y};
					#pragma unroll
					for (int k = 0; k < 4; k++) {
						const uint32_t yb = __builtin_bit_cast(uint32_t, ys[k]);
						asm("v_lshlrev_b16 %0, 4, %1" : "=v"(at[k]) : "v"(yb));     /* upper half of the result: zero */
						if constexpr (CHECK) {
							uint32_t k_abs = (uint32_t)((int)(yb - m_bits) + rfloor[cl] + tfl[a + k]);      /* yb - m_bits = round(p) */
							at[k] = k_abs < ulast ? at[k] + (uint32_t)k * W * 16u : (stage_elements + 2u) * 16u;
							window_left |= __builtin_amdgcn_ballot_w64((yb - m_bits) > W - 2u) != 0ull;      /* (wave uniform: a scalar) never, unless plan_staged's bound is wrong */
						}
					}
					#pragma unroll
					for (int k = 0; k < 4; k++) tap[k] = *(lds_f32x4 *)(uintptr_t)(at[k] + (CHECK ? 0u : (uint32_t)k * W * 16u));   /* immediate */
					const float q0 = term(f32x2{cs01.x, cs01.y}, p01.x, tap[0]);
					const float q1 = term(f32x2{cs01.z, cs01.w}, p01.y, tap[1]);
					const float q2 = term(f32x2{cs23.x, cs23.y}, p23.x, tap[2]);
					const float q3 = term(f32x2{cs23.z, cs23.w}, p23.y, tap[3]);
					if constexpr (CW) { mag2 += f32x2{q0, q1}; mag2 += f32x2{q2, q3}; }
				}
				if constexpr (CHECK) { if (window_left) staged_violation_raise(); }
			};
			if (wave_safe) batches(std::false_type{});
			else           batches(std::true_type{});
			/* per-channel fold, written scalar (hipcc otherwise builds it from packed ops and six register moves) */
			float sum_x = acc1.x - acc2.y, sum_y = acc1.y + acc2.x;
			asm volatile("" : "+v"(sum_x), "+v"(sum_y));
			const f32x4 r = *(volatile lds_f32x4 *)(uintptr_t)((uint32_t)(uintptr_t)(lds_f32x4 *)Rl + (uint32_t)cl * U * 16u);
			coherent.x = __builtin_fmaf(sum_x, r.y, __builtin_fmaf(-sum_y, r.z, coherent.x));
			coherent.y = __builtin_fmaf(sum_x, r.z, __builtin_fmaf(sum_y, r.y, coherent.y));
			if constexpr (CW) incoherent = __builtin_fmaf(__builtin_fabsf(r.w), mag2.x + mag2.y, incoherent);
		}
	}
	if (q.depth_major & 2u) staged_violation_report(tid);      /* (block uniform: every thread reaches it) */
	if (!inside) return;

	uint32_t x, y, lu_unused, lv_unused, thread = tid;
	asm volatile("" : "+v"(thread));                      /* not the values computed before the loop */
	rca_voxel_of(thread, u_axis, U, q.u_shift, V, VS, tu, tv, x, y, lu_unused, lv_unused);
	rca_store_voxel<CW>(p, zl, x, y, coherent, incoherent);
}

/* ---- the channel-paired form (q.uniform = 2): 32 x 32 tiles, 32-sample windows, 1024 threads -- the shape of config 4, whose delay
 * spread does not fit a 64-wide tile's window.  Lane l of wave w beamforms rows w and w + 16 of the tile at u = l & 31, for the
 * channel of parity h = l >> 5 of each channel pair: all 64 lanes of a wave share ONE PAIR of transmit-axis rows, so the transmit
 * delays and phasors are wave uniform again and come from a global table (staged_tables_kernel, row-pair layout) through scalar
 * loads as in UNI; and the two rows share the lane's receive position, so one packed add with the table's {T_A, T_B} forms both
 * voxels' positions.  Per round (channel pair, group of transmits) the LDS holds for every transmit of the group a 64-element block:
 * channel 2k's window, then channel 2k + 1's; the half offset h * W rides in the lane's receive entry and the lines are kept in the
 * coordinate 1/2 - (e mod 64), so the tap address is still one 16-bit shift of y = p + M (group * 64 + 2 < 4096:
 * BF_STAGED_PAIRED_GROUP_MAX).  After each channel pair lanes l and l + 32 hold the even- and the odd-channel terms of the same two
 * voxels: one exchange (v_permlane32_swap) per value and each half accumulates one of the voxels.
 * LDS: stage[a*64 + h*32 + j] (a < group), a zero element behind the largest group, R[cl*32 + u] for the chunk's channels (an odd
 * last channel gets a zero partner), tfl[A4], rfloor[chunk], rbase[chunk] (bf_staged_paired_lds_bytes, bf_kernels.h). */
template <bool CW, int NL>
__device__ __forceinline__ void staged_paired_body(const BfDasArgs &p, const BfSeparableArgs &q)
{
	extern __shared__ __attribute__((aligned(16))) f32x4 staged_lds[];
	constexpr uint32_t U = 32, W = 32, B = 2 * W;
	const int C = p.channel_count, A = p.acquisition_count, S = p.sample_count;
	const uint32_t A4 = ((uint32_t)A + 3u) & ~3u;
	const int chunk = (int)q.channel_chunk;
	/* the groups of transmits staged one after the other: G0 then G1 (0: one group).  NL: staging passes of G0, the larger */
	uint32_t G0, G1;
	if (!bf_staged_paired_split(A4, q.channel_chunk, &G0, &G1)) return;     /* (the launcher refused such a launch) */
	const uint32_t ngroups = G1 ? 2u : 1u;
	f32x4 *stage  = staged_lds + 2;                          /* (two unused elements in front, as staged_body) */
	f32x4 *R      = stage + (size_t)G0 * B + 1;
	int   *tfl    = reinterpret_cast<int *>(R + (size_t)((chunk + 1) & ~1) * U);
	int   *rfloor = tfl + A4;
	uint32_t *rbase = reinterpret_cast<uint32_t *>(rfloor + ((chunk + 2) & ~1));   /* per channel of the chunk: byte offset of its window's first sample in transmit 0's row */

	uint32_t tu, tv, zl;
	if (!staged_tile_of(q, true, tu, tv, zl)) return;        /* whole block */
	const uint32_t z = p.z_first + zl;
	const uint32_t u_axis = q.u_axis, v_axis = 1u - q.u_axis;
	const bool rx_rows = (p.transmits[0].flags & BF_RX_ROWS) != 0;
	const uint32_t tid = threadIdx.x;
	if (q.depth_major & 2u) staged_violation_clear(tid);
	/* the thread index through an opaque copy: values derived from it per chunk, pair or round are rebuilt there rather than held
	 * across the channel loop (register budget: 64 at 8 waves per SIMD) */
	auto opaque_tid = [&]() -> uint32_t { uint32_t t = tid; asm volatile("" : "+v"(t)); return t; };

	/* the tile's slice of the global table: [A4] floors, {lo, hi} of the absolute delays, then per row pair w < 16 and batch of 2
	 * transmits 48 bytes: {T''_A, T''_B of a, of a + 1}, {cos, sin}_A, {cos, sin}_B of a, the same of a + 1 */
	const unsigned char *tile_tab = reinterpret_cast<const unsigned char *>(q.tables) + (size_t)(zl * q.tiles[1] + tv) * q.table_stride;
	typedef __attribute__((address_space(4))) const int const_int;
	const_int *tab_floor = (const_int *)(uintptr_t)tile_tab;
	for (uint32_t a = tid; a < A4; a += 1024u) tfl[a] = reinterpret_cast<const int *>(tile_tab)[a];
	if (tid == 0) stage[(size_t)G0 * B] = f32x4{0.f, 0.f, 0.f, 0.f};
	f32x2 range = *reinterpret_cast<const f32x2 *>(tile_tab + 4u * A4);
	{
		const float lo = range.x, hi = range.y;              /* (scalar temporaries: see staged_uniform_range, das_staged_shared.h) */
		range.x = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, lo)));
		range.y = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, hi)));
	}

	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
	const uint32_t h = (tid >> 5) & 1u, lu = tid & 31u;
	/* a lane's voxels: rows w and w + 16 at u; row w + 16 is inside only if row w is.  A wave with no voxel inside skips the arithmetic
	 * (wave uniform: the pair's exchange below needs all 64 lanes); lanes outside the grid of a partly inside wave compute voxels of
	 * the tile that are never stored -- inside the tile, so inside the host's window bound */
	bool inside;
	{
		const uint32_t gu = tu * U + lu, gv = tv * 32u + wave;
		inside = gu < p.size[u_axis] && gv < p.size[v_axis];
	}
	const bool wave_inside = __builtin_amdgcn_ballot_w64(inside) != 0ull;

	/* Staging: per round thread tid copies element e = tid + n * 1024 (n < NL) of the group's blocks: transmit a0 + e / 64 -- wave
	 * uniform -- channel 2k + h, sample rfloor + floor(tmin_a) + (tid & 31).  lane_at: the lane's part of the byte offset, per
	 * channel pair; a missing odd channel points out of the buffer (zeros). */
	const __amdgpu_buffer_rsrc_t rf_rsrc = __builtin_amdgcn_make_buffer_rsrc(
		const_cast<void *>(p.rf), 0, (int)((uint32_t)C * (uint32_t)A * (uint32_t)S * 8u), 0x00020000);
	auto lane_at_of = [&](int cl) -> uint32_t { return rbase[cl] + ((opaque_tid() & 31u) << 3); };
	/* The wave's part of the offset is the same in every round of the tile: (a S + floor(tmin_a)) 8 for the transmit a = a0 + wave + 16 n
	 * of pass n of group g.  It is formed ONCE per tile and kept in scalars (NL per group), so a round's pass costs one add to the
	 * lane's offset -- added, not handed to the buffer load as its scalar offset: transmit 0's floor can be negative, and a scalar
	 * operand that wraps past 4 GiB is not covered by anything this kernel relies on.  A pass the wave does not own -- its transmit
	 * lies outside the group, or is one of the padding (the loop below stops at the last real transmit, so nobody
	 * reads such a block) -- is marked by bit 2 (the offsets are multiples of 8): its conversion and store are left by a scalar
	 * branch, so a group of 28 costs its slowest wave two passes and no wave a pass whose elements nobody keeps; its load is issued
	 * all the same, 2 GiB further (the host refuses inputs of 2 GiB and more here: such an offset lies outside the buffer and returns
	 * zeros without a memory access, or, where a missing odd channel's 2 GiB wrap it around, inside it: nothing is kept either way).
	 * A branch around the load would make the staging registers meet behind it: moves in every round. */
	constexpr uint32_t STAGE_SKIP = 0x80000004u;
	uint32_t stage_off[2][NL];
	#pragma unroll
	for (int g = 0; g < 2; g++) {
		const uint32_t a0 = g ? G0 : 0u, gn = g ? G1 : G0;
		#pragma unroll
		for (int n = 0; n < NL; n++) {
			const uint32_t al = wave + (uint32_t)n * 16u, a = a0 + al;
			const int fl = tab_floor[a < A4 ? a : A4 - 1u];                        /* (an index that always lies in the table) */
			uint32_t off = (a * (uint32_t)S + (uint32_t)fl) * 8u;
			if (a >= (uint32_t)A) off = STAGE_SKIP;                               /* padding: not staged */
			if (al >= gn) off = STAGE_SKIP;
			off = (uint32_t)__builtin_amdgcn_readfirstlane((int)off);
			asm volatile("" : "+s"(off));                                         /* formed here, not again in every round */
			stage_off[g][n] = off;
		}
	}
	auto stage_load = [&](uint32_t lane_at, uint32_t g, f32x2 (&regs)[NL]) {
		#pragma unroll
		for (int n = 0; n < NL; n++) {
			const uint32_t off = g ? stage_off[1][n] : stage_off[0][n];
			i32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rf_rsrc, (int)(lane_at + off), 0, 0);
			regs[n] = __builtin_bit_cast(f32x2, v);
		}
	};
	auto stage_store = [&](uint32_t g, const f32x2 (&regs)[NL]) {
		const uint32_t tid = opaque_tid();
		const float half_minus_j = 0.5f - (float)(tid & 63u);  /* the line of element e in the coordinate 1/2 - (e mod 64) */
		#pragma unroll
		for (int n = 0; n < NL; n++) {
			uint32_t off = g ? stage_off[1][n] : stage_off[0][n];
			asm volatile("" : "+s"(off));                                         /* tested here: not six branch conditions held across the rounds */
			if (off & 4u) break;                                                  /* (wave uniform; the passes a wave owns come first) */
			const float sx = regs[n].x, sy = regs[n].y;
			const float nx = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, sx), 0x130, 0xf, 0xf, true));
			const float ny = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, sy), 0x130, 0xf, 0xf, true));
			const float dx = nx - sx, dy = ny - sy;
			stage[tid + (uint32_t)n * 1024u] = f32x4{__builtin_fmaf(half_minus_j, dx, sx), __builtin_fmaf(half_minus_j, dy, sy), dx, dy};
		}
	};

	f32x2 coherent   = {0.f, 0.f};                         /* the lane's voxel after the exchanges: row w (l < 32), row w + 16 (l >= 32) */
	float incoherent = 0.f;
	/* lanes l and l + 32 hold the even and the odd channel's sums of the same two voxels {x of voxel A, y of voxel B}: after one
	 * exchange (v_permlane32_swap) lane l holds A's two, lane l + 32 B's two */
	auto exchange = [](float x, float y) -> float {
		const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, x), __builtin_bit_cast(uint32_t, y), false, false);
		return __builtin_bit_cast(float, (uint32_t)r[0]) + __builtin_bit_cast(float, (uint32_t)r[1]);
	};
	/* the lane's receive entry of pair k, R[2k * U + (tid & 63)], as an LDS byte address: rebuilt where it is read (once for the pair's
	 * mode and delay, once for its fold) rather than held in a vector register across the rounds */
	uint32_t r_base = (uint32_t)(uintptr_t)(lds_f32x4 *)R;
	asm("" : "+s"(r_base));
	auto entry_of = [&](int k) -> uint32_t { return r_base + (uint32_t)k * (2u * U * 16u) + ((opaque_tid() & 63u) << 4); };
	const uint32_t ulast = (uint32_t)(S - 1);
	const const_f32x4 *rows = (const_f32x4 *)(uintptr_t)(tile_tab + 4u * A4 + 16u) + (size_t)wave * (A4 / 2u) * 3u;

	typedef __attribute__((address_space(4))) const BfDasArgs const_args;
	const_args *kernel_args = (const_args *)__builtin_amdgcn_kernarg_segment_ptr();
	for (int c0 = 0; c0 < C; c0 += chunk) {
		const int cn = (C - c0) < chunk ? (C - c0) : chunk;
		const int cn2 = (cn + 1) & ~1;                       /* rows of the receive table: an odd last channel gets a zero partner */
		__syncthreads();        /* readers of the previous chunk's R / stage are done; tfl is complete */
		{
		const_args *ka = kernel_args;                        /* (through the kernel-argument segment: see staged_receive_table, das_staged_shared.h) */
		asm volatile("" : "+s"(ka));
		const uint32_t k_size[3] = {ka->size[0], ka->size[1], ka->size[2]};
		const float k_denom_u = fmaxf(1.0f, (float)k_size[u_axis] - 1.0f);
		uint32_t k_z = z;                                    /* (opaque: (float)z is formed here, not held in a vector register across the chunks) */
		asm volatile("" : "+s"(k_z));
		const float k_pz = (float)k_z / fmaxf(1.0f, (float)k_size[2] - 1.0f);
		const float k_fs = ka->sampling_frequency, k_inv_c = ka->inv_speed_of_sound, k_c = ka->speed_of_sound, k_fnum = ka->f_number;
		const float k_phase = ka->demodulation_frequency * ka->inv_sampling_frequency;
		const float k_pitch = rx_rows ? ka->pitch[1] : ka->pitch[0];
		for (uint32_t e = opaque_tid(); e < (uint32_t)cn2 * U; e += 1024u) {
			uint32_t cl = e >> 5, iu = e & (U - 1);
			f32x4 entry = {0.f, 0.f, 0.f, 0.f};
			if ((int)cl < cn) {
				uint32_t c = (uint32_t)c0 + cl;
				float coord[3] = {0.f, 0.f, k_pz};
				coord[u_axis] = (float)(tu * U + iu) / k_denom_u;
				float wx, wy, wz, xx, xy, xz;
				m4_point(ka->voxel_transform, coord[0], coord[1], coord[2], wx, wy, wz);
				m4_point(ka->xdc_transform, wx, wy, wz, xx, xy, xz);
				float lateral = rx_rows ? xy : xx;
				float dx      = lateral - (float)c * k_pitch;
				float a_arg   = __builtin_fabsf(dx * (k_fnum * hw_rcp(__builtin_fabsf(xz))));
				float r_idx = div_speed_of_sound(hw_sqrt(dx * dx + xz * xz), k_inv_c, k_c) * k_fs;
				entry.x = r_idx;
				if (a_arg < 0.5f) {
					float cs    = hw_cos_turns(0.5f * a_arg);
					float apod  = cs * cs;
					float turns = phase_turns(k_phase, r_idx);
					entry.y = apod * hw_cos_turns(turns);
					entry.z = apod * hw_sin_turns(turns);
					entry.w = apod;
				}
			}
			R[e] = entry;
		}
		}
		__syncthreads();
		for (uint32_t cl = opaque_tid(); cl < (uint32_t)cn2; cl += 1024u) {
			const float *row = reinterpret_cast<const float *>(R + (size_t)cl * U);
			float m = row[0];
			#pragma unroll 4
			for (uint32_t iu = 1; iu < U; iu++) m = fminf(m, row[4 * iu]);
			const int fl = (int)__builtin_floorf(m);
			rfloor[cl] = fl;
			/* (a missing odd channel points out of the buffer and stays there with a lane's and a transmit's offset added: the host
			 * refuses inputs of 2 GiB and more) */
			rbase[cl] = c0 + (int)cl < C ? ((uint32_t)(c0 + (int)cl) * (uint32_t)A * (uint32_t)S + (uint32_t)fl) * 8u : 0x80000000u;
		}
		__syncthreads();
		/* window-relative delay plus the half offset h * W of the lane's window in the block; the sign of the weight: the lane may leave
		 * the RF row for some transmit of the tile (the zero partner of an odd channel never does) */
		int k_last = S - 1;                                  /* (opaque, as k_z above: the float is formed per chunk, not held across them) */
		asm volatile("" : "+s"(k_last));
		for (uint32_t e = opaque_tid(); e < (uint32_t)cn2 * U; e += 1024u) {
			f32x4 entry = R[e];
			const uint32_t cl = e >> 5;
			const bool lane_safe = (int)cl >= cn || ((entry.x + range.x >= 0.f) && (entry.x + range.y < (float)k_last));
			entry.x = (entry.x - (float)rfloor[cl]) + (float)((cl & 1u) * W);     /* both steps exact */
			if (!lane_safe) entry.w = -entry.w;
			R[e] = entry;
		}
		__syncthreads();

		/* What a wave does with a channel pair: nothing (no voxel inside, or the f-number culls both channels for every lane), the plain
		 * loop, or the range-checked one -- decided once per pair from the lane's receive entry, whose delay the pair's rounds use. */
		const int pairs = cn2 / 2;
		auto mode_of = [&](int k, float &r_rel) -> int {
			if (!wave_inside) return 0;
			const __attribute__((address_space(3))) float *r = (const __attribute__((address_space(3))) float *)(uintptr_t)entry_of(k);
			const float r_w = r[3];                                            /* (two words of the entry, not the four) */
			r_rel = r[0];
			if (__builtin_amdgcn_ballot_w64(r_w != 0.f) == 0) return 0;        /* F# culling per wave (both channels of the pair) */
			return (!(q.depth_major & 2u) && __builtin_amdgcn_ballot_w64(__builtin_signbitf(r_w)) == 0) ? 1 : 2;
		};
		float r_rel = 0.f;
		int k = 0, mode = mode_of(0, r_rel);
		/* A RUN of pairs: the pairs from k on for as long as the wave's mode stays MODE, at most to the end of the chunk.  The aperture
		 * is a contiguous range of channels, so a wave's mode changes a handful of times over a frame's pairs; with the pair loop inside
		 * the case the staging registers and the voxel's sums stay where they are from pair to pair, and the three cases meet once per
		 * run instead of once per pair.  Every wave executes the same sequence of rounds whatever its mode: the barriers are block
		 * uniform.  The staging registers belong to the run: it requests its first pair's windows itself, and its last pair requests
		 * nothing -- the next pair's case is looked up at the top of a pair, before the round where the request would stand --, so no
		 * load is in flight where two cases meet (a few times per tile, against a chunk's own first request once per chunk). */
		auto run = [&](auto mode_c) {
			constexpr int MODE = decltype(mode_c)::value;
			constexpr bool CHECK = MODE == 2;
			/* the plain loop fetches the next batch's table row ahead (below); the range-checked loop and the four-pass instance have
			 * no register for that order and read a batch's row at its top */
			constexpr bool AHEAD = MODE == 1 && NL <= 3;
			f32x2 regs[NL] = {};
			stage_load(lane_at_of(2 * k + (int)h), 0, regs);
			do {
				float next_rel = 0.f;
				int next_mode = -1;                              /* (behind the chunk's last pair: no case) */
				if (k + 1 < pairs) next_mode = mode_of(k + 1, next_rel);
				f32x2 acc1a = {0.f, 0.f}, acc2a = {0.f, 0.f}, acc1b = {0.f, 0.f}, acc2b = {0.f, 0.f};
				f32x2 mag2 = {0.f, 0.f};                         /* {voxel A, voxel B} */
				for (uint32_t g = 0; g < ngroups; g++) {
					__syncthreads();               /* everyone is done with the previous round's windows */
					stage_store(g, regs);
					__syncthreads();
					if (g + 1 < ngroups) stage_load(lane_at_of(2 * k + (int)h), 1, regs);         /* in flight during the arithmetic */
					else if (next_mode == MODE) stage_load(lane_at_of(2 * k + 2 + (int)h), 0, regs);
					if constexpr (MODE != 0) {
						const uint32_t a0 = g ? G0 : 0u, gn = g ? G1 : G0;
						/* the transmits the round runs: the group's, or only its real ones (the padding of the count to a multiple of 4
						 * sits at the end of the last group: zero phasors over zero windows, 1/76 of config 4's terms) */
						const uint32_t left = (uint32_t)A - a0, gr = left < gn ? left : gn;
						/* position -> tap as staged_body; M = 2^23 + 2 + (the batch's first block) * 64, the lane's window starts h * W
						 * further (its receive entry carries that offset) */
						uint32_t m_bits = 0x4B000002u;
						[[maybe_unused]] bool window_left = false;
						[[maybe_unused]] int rfl_h = 0;                          /* checked loop: rfloor of the lane's channel - h * W */
						if constexpr (CHECK) rfl_h = rfloor[2 * k + (int)h] - (int)(h * W);
						const f32x2 rr = {r_rel, r_rel};
						/* One batch: two transmits, four terms a lane ({A, B} of transmit a, of a + 1), from one table row: positions, tap
						 * addresses, the LDS reads, then per term interpolation, rotate-accumulate and magnitude.  AHEAD: all rotate-accumulates
						 * first -- behind them the row is dead --, `behind_rotates`, then the four magnitudes.  (Each accumulator sees its
						 * terms in the same order either way: the same bits.)  PART: both transmits of the row, or only its first or its second
						 * -- the same body, so that a group of an odd number of real transmits ends in the pair path's own registers. */
						auto batch = [&](auto part_c, uint32_t a, const f32x4 tz, const f32x4 cs0, const f32x4 cs1, auto &&behind_rotates) {
							constexpr int PART = decltype(part_c)::value;
							constexpr int T0 = PART == 2 ? 2 : 0, T = PART == 1 ? 2 : 4;      /* terms T0 .. T - 1 */
							uint32_t at[4]; f32x4 tap[4]; f32x2 sv[4];
							const float M = __builtin_bit_cast(float, m_bits);
							const f32x2 M2 = {M, M};
							const f32x2 p0 = rr + f32x2{tz.x, tz.y}, p1 = rr + f32x2{tz.z, tz.w};
							const f32x2 y0 = p0 + M2, y1 = p1 + M2;
							const float ys[4] = {y0.x, y0.y, y1.x, y1.y}, ps[4] = {p0.x, p0.y, p1.x, p1.y};
							const f32x2 cs[4] = {{cs0.x, cs0.y}, {cs0.z, cs0.w}, {cs1.x, cs1.y}, {cs1.z, cs1.w}};
							#pragma unroll
							for (int t = T0; t < T; t++) {
								const uint32_t yb = __builtin_bit_cast(uint32_t, ys[t]);
								asm("v_lshlrev_b16 %0, 4, %1" : "=v"(at[t]) : "v"(yb));
								if constexpr (CHECK) {
									uint32_t lane_id = tid;
									asm volatile("" : "+v"(lane_id));                            /* h * W = tid & 32, not held across the loop */
									const uint32_t rel = yb - m_bits;                             /* round(p) in the transmit's block */
									const uint32_t k_abs = (uint32_t)((int)rel + rfl_h + tfl[a0 + a + (uint32_t)(t >> 1)]);
									at[t] = k_abs < ulast ? at[t] + (uint32_t)(t >> 1) * B * 16u : (G0 * B + 2u) * 16u;
									window_left |= __builtin_amdgcn_ballot_w64(inside && rel - (lane_id & 32u) > W - 2u) != 0ull;   /* (voxels in the grid) */
								}
							}
							#pragma unroll
							for (int t = T0; t < T; t++) tap[t] = *(lds_f32x4 *)(uintptr_t)(at[t] + (CHECK ? 0u : (uint32_t)(t >> 1) * B * 16u));
							[[maybe_unused]] float q[4] = {0.f, 0.f, 0.f, 0.f};
							#pragma unroll
							for (int t = T0; t < T; t++) {
								sv[t] = f32x2{tap[t].x, tap[t].y} + ps[t] * f32x2{tap[t].z, tap[t].w};
								if (t & 1) { acc1b += sv[t].x * cs[t]; acc2b += sv[t].y * cs[t]; }
								else       { acc1a += sv[t].x * cs[t]; acc2a += sv[t].y * cs[t]; }
								if constexpr (CW && !AHEAD) q[t] = hw_sqrt(__builtin_fmaf(sv[t].y, sv[t].y, sv[t].x * sv[t].x));
							}
							behind_rotates();
							if constexpr (CW) {
								#pragma unroll
								for (int t = T0; AHEAD && t < T; t++) q[t] = hw_sqrt(__builtin_fmaf(sv[t].y, sv[t].y, sv[t].x * sv[t].x));
								if constexpr (T0 == 0) mag2 += f32x2{q[0], q[1]};
								if constexpr (T == 4)  mag2 += f32x2{q[2], q[3]};
							}
						};
						constexpr std::integral_constant<int, 0> both{};
						constexpr std::integral_constant<int, 1> first{};
						constexpr std::integral_constant<int, 2> second{};
						const_f32x4 *row = rows + (size_t)(a0 / 2u) * 3u;
						uint32_t a = 0;
						if constexpr (!AHEAD) {
							for (; a + 1u < gr; a += 2, m_bits += 2u * B, row += 3) batch(both, a, row[0], row[1], row[2], [] {});
							if (a < gr) batch(first, a, row[0], row[1], row[1], [] {});
						} else {
							/* The plain loop asks for the NEXT batch's row where this batch's row dies, behind the last rotate-accumulate: the
							 * twelve scalars are reloaded in place and the magnitudes cover the scalar loads' latency, so the wait at the top
							 * of a batch finds them there.  The group's last row stands behind the loop and asks for nothing: every row requested
							 * is a row of the group.  It is written as its first transmit and, if that is a real one, its second: written as
							 * "a pair or one transmit" hipcc computes the common half once into new registers and copies four sums back. */
							f32x4 tz = row[0], cs0 = row[1], cs1 = row[2];
							for (; a + 2u < gr; a += 2, m_bits += 2u * B)
								batch(both, a, tz, cs0, cs1, [&] {
									__builtin_amdgcn_sched_barrier(0);
									row += 3;
									tz = row[0]; cs0 = row[1]; cs1 = row[2];
									__builtin_amdgcn_sched_barrier(0);
								});
							batch(first, a, tz, cs0, cs1, [] {});
							if (a + 1u < gr) batch(second, a, tz, cs0, cs1, [] {});
						}
						if constexpr (CHECK) { if (window_left) staged_violation_raise(); }
					}
				}
				if constexpr (MODE != 0) {
					/* the pair's fold: the lane's channel's term of both voxels, then the two channels of the pair summed per voxel */
					float sa_x = acc1a.x - acc2a.y, sa_y = acc1a.y + acc2a.x;
					float sb_x = acc1b.x - acc2b.y, sb_y = acc1b.y + acc2b.x;
					asm volatile("" : "+v"(sa_x), "+v"(sa_y), "+v"(sb_x), "+v"(sb_y));
					const f32x4 r = *(volatile lds_f32x4 *)(uintptr_t)entry_of(k);
					const float ca_x = __builtin_fmaf(sa_x, r.y, -sa_y * r.z), ca_y = __builtin_fmaf(sa_x, r.z, sa_y * r.y);
					const float cb_x = __builtin_fmaf(sb_x, r.y, -sb_y * r.z), cb_y = __builtin_fmaf(sb_x, r.z, sb_y * r.y);
					coherent.x += exchange(ca_x, cb_x);
					coherent.y += exchange(ca_y, cb_y);
					if constexpr (CW) incoherent += exchange(__builtin_fabsf(r.w) * mag2.x, __builtin_fabsf(r.w) * mag2.y);
				}
				k++;
				mode = next_mode;
				/* (the four-pass instance has no register to carry the next pair's delay through the round: it reads it again) */
				if constexpr (NL >= 4) next_rel = mode > 0 ? *(volatile __attribute__((address_space(3))) float *)(uintptr_t)entry_of(k) : 0.f;
				r_rel = next_rel;
			} while (mode == MODE);
		};
		while (k < pairs) {
			if (mode == 1)      run(std::integral_constant<int, 1>{});
			else if (mode == 2) run(std::integral_constant<int, 2>{});
			else                run(std::integral_constant<int, 0>{});
		}
	}
	if (q.depth_major & 2u) staged_violation_report(tid);      /* (block uniform: every thread reaches it) */
	uint32_t thread = tid;
	asm volatile("" : "+v"(thread));                      /* not the values computed before the loop */
	const uint32_t gu = tu * U + (thread & 31u), gv = tv * 32u + (thread >> 6) + ((thread >> 5) & 1u) * 16u;
	if (!(gu < p.size[u_axis] && gv < p.size[v_axis])) return;
	const uint32_t x = u_axis == 0 ? gu : gv, y = u_axis == 0 ? gv : gu;
	uint64_t out_index = (uint64_t)p.size[0] * p.size[1] * zl + (uint64_t)p.size[0] * y + x;
	reinterpret_cast<f32x2 *>(p.out)[out_index] = coherency_weighted<CW>(coherent, incoherent);
}

template <bool CW, int VS, int WS, int NL, bool UNI, bool PAIRED>
__global__ __launch_bounds__(1024, 8) void das_rca_staged_kernel(const BfDasArgs p, const BfSeparableArgs q)
{
	if constexpr (PAIRED) staged_paired_body<CW, NL>(p, q);
	else                  staged_body<CW, VS, WS, NL, UNI>(p, q);
}

template <bool CW>
static hipError_t launch_staged_shape(const BfDasArgs *a, const BfSeparableArgs *q, hipStream_t s)
{
	/* the paired walk (depth_major bit 2, global tables only) pads the planes to chunks of 32 */
	const uint32_t tiles = q->tiles[0] * q->tiles[1] * q->tiles[2];
	const uint32_t tiles_padded = (q->depth_major & 4u) ? q->tiles[0] * q->tiles[1] * ((q->tiles[2] + 31u) >> 5) * 32u : tiles;
	if (q->uniform == 2) {
		/* the channel-paired form: 32 x 32 tiles, 32-sample windows, 1024 threads, an even chunk of channels (or all of them) */
		if (q->u_shift != 5 || q->v_shift != 5 || q->window_samples != 32 || q->threads != 1024 || !q->tables ||
		    ((q->channel_chunk & 1u) && (int)q->channel_chunk < a->channel_count)) return hipErrorInvalidValue;
		const uint32_t A4 = ((uint32_t)a->acquisition_count + 3u) & ~3u;
		uint32_t G0, G1;
		if (!bf_staged_paired_split(A4, q->channel_chunk, &G0, &G1) || q->lds_bytes < bf_staged_paired_lds_bytes(G0, q->channel_chunk, A4)) return hipErrorInvalidValue;
		switch (bf_staged_paired_passes(G0)) {               /* staging passes of the larger group; the other one's are bounded in the kernel */
		case 2: return rca_launch_tiles(das_rca_staged_kernel<CW, 5, 5, 2, true, true>, tiles_padded, 1024u, a, q, s);
		case 3: return rca_launch_tiles(das_rca_staged_kernel<CW, 5, 5, 3, true, true>, tiles_padded, 1024u, a, q, s);
		case 4: return rca_launch_tiles(das_rca_staged_kernel<CW, 5, 5, 4, true, true>, tiles_padded, 1024u, a, q, s);
		}
		return hipErrorInvalidValue;
	}
	if (q->uniform) {
		/* wave-uniform transmit tables: a 64 x 16 tile with x along the receive axis, 1024 threads, tables written by bf_launch_das_staged_tables */
		if (q->u_axis != 0 || q->u_shift != 6 || q->v_shift != 4 || q->threads != 1024 || !q->tables) return hipErrorInvalidValue;
		auto loads = [&](auto ws) {
			constexpr int WS = decltype(ws)::value;
			return staged_for_passes(staged_passes(a, q, WS), [&](auto nl) {
				return rca_launch_tiles(das_rca_staged_kernel<CW, 4, WS, decltype(nl)::value, true, false>, tiles_padded, q->threads, a, q, s);
			});
		};
		if (q->window_samples == 32) return loads(std::integral_constant<int, 5>{});
		if (q->window_samples == 64) return loads(std::integral_constant<int, 6>{});
		return hipErrorInvalidValue;
	}
	return staged_for_shape(q, [&](auto vs, auto ws) {
		constexpr int VS = decltype(vs)::value, WS = decltype(ws)::value;
		return staged_for_passes(staged_passes(a, q, WS), [&](auto nl) {
			return rca_launch_tiles(das_rca_staged_kernel<CW, VS, WS, decltype(nl)::value, false, false>, tiles, q->threads, a, q, s);
		});
	});
}

/* complex samples, linear interpolation only; the caller checked q->window_shift */
extern "C" hipError_t bf_launch_das_staged(const BfDasArgs *a, const BfSeparableArgs *q, hipStream_t s)
{
	if (!a->complex_data || a->interpolation != BF_INTERP_LINEAR) return hipErrorInvalidValue;
	/* the staging loads address the DAS input through 32-bit buffer offsets with out-of-range padding at 2^31 */
	if ((uint64_t)a->channel_count * (uint64_t)a->acquisition_count * (uint64_t)a->sample_count * 8u >= (1ull << 31)) return hipErrorInvalidValue;
	return a->coherency_weighting ? launch_staged_shape<true>(a, q, s) : launch_staged_shape<false>(a, q, s);
}

/* ---- the transmit tables of the UNI variant, once per frame: one block per (lateral tile row tv, plane zl), the calls of the
 * kernel's own table build (same functions, same order: the entries are bit-identical to what a block would compute in LDS).
 * Layout per tile slice of q.table_stride bytes: int floor(tmin_a)[A4] | {lo, hi} of the absolute delays + 8 bytes of padding |
 * per lateral row iv < 16 and batch b < A4 / 4: {T'' of transmits 4b .. 4b + 3}, {cos, sin} of 4b, 4b + 1, {cos, sin} of 4b + 2, 4b + 3. */
template <int VS>
__global__ __launch_bounds__(256) void staged_tables_kernel(const BfDasArgs p, const BfSeparableArgs q)
{
	extern __shared__ __attribute__((aligned(16))) f32x4 tables_lds[];
	constexpr uint32_t V = 1u << VS;
	const int A = p.acquisition_count;
	const int A4 = (A + 3) & ~3;
	float *t  = reinterpret_cast<float *>(tables_lds);                 /* [A4][V] */
	f32x2 *cs = reinterpret_cast<f32x2 *>(t + (size_t)A4 * V);          /* [A4][V] */
	f32x2 *wave_range = cs + (size_t)A4 * V;                            /* [4] */
	const uint32_t tv = blockIdx.x % q.tiles[1], zl = blockIdx.x / q.tiles[1];
	const uint32_t tid = threadIdx.x, nthreads = blockDim.x;
	staged_transmit_entries<VS, true>(p, 1u - q.u_axis, tv, p.z_first + zl, tid, nthreads, [&](uint32_t, uint32_t, uint32_t e, float t_idx, float cs_c, float cs_s) {
		t[e] = t_idx; cs[e] = f32x2{cs_c, cs_s};
	});
	const f32x2 range = rca_tile_range((uint32_t)A * V, wave_range, [&](uint32_t e) { return t[e]; });
	unsigned char *tile_tab = reinterpret_cast<unsigned char *>(q.tables) + (size_t)blockIdx.x * q.table_stride;
	if (tid == 0) *reinterpret_cast<f32x4 *>(tile_tab + 4u * (uint32_t)A4) = f32x4{range.x, range.y, 0.f, 0.f};
	for (uint32_t a = tid; a < (uint32_t)A4; a += nthreads) reinterpret_cast<int *>(tile_tab)[a] = staged_window_row<V, 1, 0>(t + (size_t)a * V);
	__syncthreads();
	f32x4 *rows = reinterpret_cast<f32x4 *>(tile_tab + 4u * (uint32_t)A4 + 16u);
	if constexpr (VS == 5) {
		/* the channel-paired form: per row pair w < 16 (rows w, w + 16) and batch of 2 transmits a = 2b, a + 1 */
		const uint32_t batches = (uint32_t)A4 / 2u;
		for (uint32_t e = tid; e < 16u * batches; e += nthreads) {
			const uint32_t w = e / batches, b = e % batches;
			const float *t2 = t + (size_t)(2u * b) * V + w;
			const f32x2 *c2 = cs + (size_t)(2u * b) * V + w;
			f32x4 *row = rows + (size_t)e * 3u;
			row[0] = f32x4{t2[0], t2[16], t2[V], t2[V + 16]};
			row[1] = f32x4{c2[0].x, c2[0].y, c2[16].x, c2[16].y};
			row[2] = f32x4{c2[V].x, c2[V].y, c2[V + 16].x, c2[V + 16].y};
		}
		return;
	}
	const uint32_t batches = (uint32_t)A4 / 4u;
	for (uint32_t e = tid; e < V * batches; e += nthreads) {
		const uint32_t iv = e / batches, b = e % batches;
		const float *t4 = t + (size_t)(4u * b) * V + iv;
		const f32x2 *c4 = cs + (size_t)(4u * b) * V + iv;
		f32x4 *row = rows + (size_t)e * 3u;
		row[0] = f32x4{t4[0], t4[V], t4[2 * V], t4[3 * V]};
		row[1] = f32x4{c4[0].x, c4[0].y, c4[V].x, c4[V].y};
		row[2] = f32x4{c4[2 * V].x, c4[2 * V].y, c4[3 * V].x, c4[3 * V].y};
	}
}

/* one launch per frame and shard, before bf_launch_das_staged with q->uniform set; q->tables holds q->tiles[1] * q->tiles[2] slices */
extern "C" hipError_t bf_launch_das_staged_tables(const BfDasArgs *a, const BfSeparableArgs *q, hipStream_t s)
{
	const uint32_t A4 = ((uint32_t)a->acquisition_count + 3u) & ~3u;
	if (!q->tables) return hipErrorInvalidValue;
	if (q->uniform == 1 && q->v_shift == 4) {
		if (q->table_stride < 4u * A4 + 16u + 16u * (A4 / 4u) * 48u) return hipErrorInvalidValue;
		hipLaunchKernelGGL(staged_tables_kernel<4>, dim3(q->tiles[1] * q->tiles[2]), dim3(256), A4 * 16u * 12u + 64u, s, *a, *q);
		return hipGetLastError();
	}
	if (q->uniform == 2 && q->v_shift == 5) {
		if (q->table_stride < 4u * A4 + 16u + 16u * (A4 / 2u) * 48u) return hipErrorInvalidValue;
		const uint32_t lds = A4 * 32u * 12u + 64u;
		hipError_t e = hipFuncSetAttribute((const void *)staged_tables_kernel<5>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (e != hipSuccess) return e;
		hipLaunchKernelGGL(staged_tables_kernel<5>, dim3(q->tiles[1] * q->tiles[2]), dim3(256), lds, s, *a, *q);
		return hipGetLastError();
	}
	return hipErrorInvalidValue;
}
