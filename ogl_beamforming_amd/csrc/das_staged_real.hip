/* das_staged_real.hip -- the LDS-staged row-column DAS kernel (das_staged.hip) for REAL samples.
 *
 * Same design, half the data: pipelines without Demodulate (e.g. {Decode, DAS} on Int16 RF) hand DAS
 * real float samples, sample_rf has no IQ rotation (shaders/das.glsl:99-124 with SAMPLE_TYPE float), and
 * the coherency weight sums |sample| (das.glsl:29, length() of a scalar).  Everything das_staged.hip's
 * header explains applies -- window position in the float tables, window elements stored as lines
 * {c_j, d_j} in window coordinates (8 bytes here: ONE ds_read_b64 per term and the interpolation one fma
 * of the position itself), magic-number rounding for the tap address, transmit delays in pairs, the
 * per-lane range flag in the sign of the receive weight, buffer-load staging with the next channel's
 * windows in flight -- minus the phasor tables and the complex multiply-accumulate.  Per term the inner
 * loop is: half a packed add (position), half a packed add (rounding), one v_lshlrev_b16 (address), one
 * fma (interpolation), one add (sum), and with coherency weighting one add of |sample| (a free modifier).
 * The gather kernel (das_separable.hip) pays 16.3 clk per wave64 gather for the same term.
 */
#include "das_staged_shared.h"

/* LDS (A4 = transmits rounded up to a multiple of 4):
 *   stage[a*W + j]   = { c_j, d_j }: the line through samples j and j + 1 of window (c, a) in window coordinates;
 *                      j < W, a < A4; two unused elements in front, one zero element behind          f32x2
 *   R[cl*U + u]      = { R' = r_index - floor(rmin_c), +-apod }   (sign bit set: the lane may leave the RF row)   f32x2
 *   Tz[(a/2)*V + v]  = { T'' = t_index - floor(tmin_a) - 1/2 of transmit a & ~1, of transmit a | 1 }   f32x2
 *   tfl[a] = floor(tmin_a),  rfloor[cl] = floor(rmin_c)                                                int
 *   wave_range[16]                                                                                     f32x2 */
template <bool CW, int VS, int WS, int NL>
__global__ __launch_bounds__(1024, 8) void das_rca_staged_real_kernel(const BfDasArgs p, const BfSeparableArgs q)
{
	extern __shared__ __attribute__((aligned(16))) f32x2 staged_real_lds[];
	constexpr uint32_t V = 1u << VS, W = 1u << WS;
	const uint32_t U = 1u << q.u_shift;
	const int C = p.channel_count, A = p.acquisition_count, S = p.sample_count;
	const int A4 = (A + 3) & ~3;
	const int chunk = (int)q.channel_chunk;
	/* the staging area comes first and the kernel has no static LDS: 8 x (a window element's index + 2) IS its LDS address */
	f32x2 *stage  = staged_real_lds + 2;
	f32x2 *R      = stage + (size_t)A4 * W + 2;              /* (+ the zero element, + one to keep 16-byte alignment) */
	f32x2 *Tz     = R + (size_t)chunk * U;
	int   *tfl    = reinterpret_cast<int *>(Tz + (size_t)(A4 / 2) * V);
	int   *rfloor = tfl + A4;
	f32x2 *wave_range = reinterpret_cast<f32x2 *>(rfloor + ((chunk + 1) & ~1));
	const uint32_t stage_elements = (uint32_t)A4 * W;

	uint32_t tu, tv, zl;
	if (!staged_tile_of(q, false, tu, tv, zl)) return;      /* whole block */
	const uint32_t z  = p.z_first + zl;

	const uint32_t u_axis = q.u_axis, v_axis = 1u - q.u_axis;
	const bool  rx_rows = (p.transmits[0].flags & BF_RX_ROWS) != 0;
	const uint32_t tid = threadIdx.x, nthreads = blockDim.x;
	if (q.depth_major & 2u) staged_violation_clear(tid);       /* STAGED_CHECKED: das_common.h */

	/* ---- transmit delays: no phasors */
	staged_transmit_entries<VS, false>(p, v_axis, tv, z, tid, nthreads, [&](uint32_t a, uint32_t iv, uint32_t, float t_idx, float, float) {
		reinterpret_cast<float *>(Tz + (a >> 1) * V + iv)[a & 1u] = t_idx;
	});
	if (tid == 0) stage[stage_elements] = f32x2{0.f, 0.f};
	const f32x2 range = rca_tile_range((uint32_t)A * V, wave_range, [&](uint32_t e) {
		uint32_t a = e >> VS, iv = e & (V - 1);
		return reinterpret_cast<const float *>(Tz + (a >> 1) * V + iv)[a & 1u];
	});
	for (uint32_t a = tid; a < (uint32_t)A4; a += nthreads)
		tfl[a] = staged_window_row<V, 2, 0>(reinterpret_cast<float *>(Tz + (size_t)(a >> 1) * V) + (a & 1u));
	__syncthreads();                                         /* the floors are read below */

	uint32_t x, y, lu, lv_unused;
	rca_voxel_of(tid, u_axis, U, q.u_shift, V, VS, tu, tv, x, y, lu, lv_unused);
	const bool inside = x < p.size[0] && y < p.size[1];

	float coherent = 0.f, incoherent = 0.f;
	const f32x2   *Rl = R + lu;
	const uint32_t ulast = (uint32_t)(S - 1);
	uint32_t tz_base = (uint32_t)(uintptr_t)(lds_f32x2 *)Tz;
	asm("" : "+s"(tz_base));

	/* staging (das_staged_shared.h): 4-byte samples */
	const __amdgpu_buffer_rsrc_t rf_rsrc = staged_rf_resource<float>(p);
	uint32_t stage_inv[NL];
	staged_stage_offsets<float, WS, 0>(stage_inv, tfl, A, S, tid, nthreads);
	auto stage_load = [&](int channel, int rfl, float (&regs)[NL]) { staged_stage_load(rf_rsrc, stage_inv, channel, A, S, rfl, regs); };
	const float half_minus_j = 0.5f - (float)(tid & (W - 1));
	auto stage_store = [&](const float (&regs)[NL]) {
		#pragma unroll
		for (int n = 0; n < NL; n++) {
			const float s0 = regs[n];
			const float s1 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s0), 0x130, 0xf, 0xf, true));
			uint32_t e = tid + (uint32_t)n * nthreads;
			const float d = s1 - s0;
			if (e < stage_elements) stage[e] = f32x2{__builtin_fmaf(half_minus_j, d, s0), d};
		}
	};

	for (int c0 = 0; c0 < C; c0 += chunk) {
		const int cn = (C - c0) < chunk ? (C - c0) : chunk;
		__syncthreads();
		staged_receive_table<f32x2, 0>(R, rfloor, c0, cn, tu, z, u_axis, q.u_shift, rx_rows, range, S, tid, nthreads);

		float regs[NL];
		stage_load(c0, rfloor[0], regs);
		for (int cl = 0; cl < cn; cl++) {
			__syncthreads();
			stage_store(regs);
			__syncthreads();
			if (cl + 1 < cn) stage_load(c0 + cl + 1, rfloor[cl + 1], regs);
			if (!inside) continue;

			float r_rel, r_w;
			{
				const f32x2 r = Rl[(size_t)cl * U];
				r_rel = r.x; r_w = r.y;
			}
			if (__builtin_amdgcn_ballot_w64(r_w != 0.f) == 0) continue;    /* F# culling per wave */
			const bool wave_safe = !(q.depth_major & 2u) && __builtin_amdgcn_ballot_w64(__builtin_signbitf(r_w)) == 0;
			f32x2 sum2 = {0.f, 0.f}, mag2 = {0.f, 0.f};
			auto batches = [&](auto checked) {
				constexpr bool CHECK = decltype(checked)::value;
				uint32_t lane_id = tid;
				asm volatile("" : "+v"(lane_id));
				const uint32_t lane_v = u_axis == 0 ? lane_id >> q.u_shift : lane_id & (V - 1);
				uint32_t tz_at = tz_base + (lane_v << 3);
				uint32_t m_bits = 0x4B000002u;               /* 2^23 + 2: das_staged.hip explains the rounding and the bias */
				[[maybe_unused]] bool window_left = false;    /* range-checked loop: some term selected an element outside its window */
				const f32x2 rr = {r_rel, r_rel};
				for (int a = 0; a < A4; a += 4, tz_at += 2u * V * 8u, m_bits += 4u * W) {
					uint32_t at[4]; f32x2 tap[4];
					const float M = __builtin_bit_cast(float, m_bits);
					const f32x2 M2 = {M, M};
					const f32x2 tz01 = *(lds_f32x2 *)(uintptr_t)tz_at;
					const f32x2 tz23 = *(lds_f32x2 *)(uintptr_t)(tz_at + V * 8u);
					const f32x2 p01 = rr + tz01, p23 = rr + tz23;
					const f32x2 y01 = p01 + M2,  y23 = p23 + M2;
					const float ys[4] = {y01.x, y01.y, y23.x, y23.y}, ps[4] = {p01.x, p01.y, p23.x, p23.y};
					#pragma unroll
					for (int k = 0; k < 4; k++) {
						const uint32_t yb = __builtin_bit_cast(uint32_t, ys[k]);
						asm("v_lshlrev_b16 %0, 3, %1" : "=v"(at[k]) : "v"(yb));
						if constexpr (CHECK) {
							uint32_t k_abs = (uint32_t)((int)(yb - m_bits) + rfloor[cl] + tfl[a + k]);      /* yb - m_bits = round(p) */
							at[k] = k_abs < ulast ? at[k] + (uint32_t)k * W * 8u : (stage_elements + 2u) * 8u;
							window_left |= __builtin_amdgcn_ballot_w64((yb - m_bits) > W - 2u) != 0ull;      /* (wave uniform: a scalar) never, unless plan_staged's bound is wrong */
						}
					}
					#pragma unroll
					for (int k = 0; k < 4; k++) tap[k] = *(lds_f32x2 *)(uintptr_t)(at[k] + (CHECK ? 0u : (uint32_t)k * W * 8u));   /* immediate */
					float sv[4];
					#pragma unroll
					for (int k = 0; k < 4; k++) {
						sv[k] = __builtin_fmaf(ps[k], tap[k].y, tap[k].x);
						asm("" : "+v"(sv[k]));       /* four plain fmas: packed, hipcc spends six moves pairing their operands */
					}
					sum2 += f32x2{sv[0], sv[1]}; sum2 += f32x2{sv[2], sv[3]};
					if constexpr (CW) {
						mag2 += f32x2{__builtin_fabsf(sv[0]), __builtin_fabsf(sv[1])};
						mag2 += f32x2{__builtin_fabsf(sv[2]), __builtin_fabsf(sv[3])};
					}
				}
				if constexpr (CHECK) { if (window_left) staged_violation_raise(); }
			};
			if (wave_safe) batches(std::false_type{});
			else           batches(std::true_type{});
			const float apod = __builtin_fabsf(r_w);
			coherent = __builtin_fmaf(sum2.x + sum2.y, apod, coherent);
			if constexpr (CW) incoherent = __builtin_fmaf(mag2.x + mag2.y, apod, incoherent);
		}
	}
	if (q.depth_major & 2u) staged_violation_report(tid);      /* (block uniform: every thread reaches it) */
	if (!inside) return;

	rca_store_voxel<CW>(p, zl, x, y, coherent, incoherent);
}

template <bool CW>
static hipError_t launch_staged_real_shape(const BfDasArgs *a, const BfSeparableArgs *q, hipStream_t s)
{
	return staged_for_shape(q, [&](auto vs, auto ws) {
		constexpr int VS = decltype(vs)::value, WS = decltype(ws)::value;
		auto launch = [&](auto nl) {
			return rca_launch_tiles(das_rca_staged_real_kernel<CW, VS, WS, decltype(nl)::value>, q->tiles[0] * q->tiles[1] * q->tiles[2], q->threads, a, q, s);
		};
		const uint32_t passes = staged_passes(a, q, WS);
		switch (passes) {
		case 5: case 6: return launch(std::integral_constant<int, 6>{});       /* (a staging width larger than needed only loads zeros) */
		case 7: case 8: return launch(std::integral_constant<int, 8>{});
		}
		return staged_for_passes(passes, launch);
	});
}

/* real samples, linear interpolation; the caller (bf_launch_das_staged) checked the rest */
extern "C" hipError_t bf_launch_das_staged_real(const BfDasArgs *a, const BfSeparableArgs *q, hipStream_t s)
{
	if (a->complex_data || a->interpolation != BF_INTERP_LINEAR) return hipErrorInvalidValue;
	if ((uint64_t)a->channel_count * (uint64_t)a->acquisition_count * (uint64_t)a->sample_count * 4u >= (1ull << 31)) return hipErrorInvalidValue;
	return a->coherency_weighting ? launch_staged_real_shape<true>(a, q, s) : launch_staged_real_shape<false>(a, q, s);
}
