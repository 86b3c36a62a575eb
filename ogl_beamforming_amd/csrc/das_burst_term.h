/* das_burst_term.h -- what the three kernels of das_burst.hip and das_burst_views.hip share beyond das_general.h: the frames of a block
 * (burst_frames) and one term of BF_BURST_FRAMES_PER_THREAD frames (burst_term).  The RCA loop around the term is restated in
 * das_burst_kernel and das_burst_views_kernel: shared as a function it compiled to other code in both (das_burst_views.hip). */
#ifndef BF_DAS_BURST_TERM_H
#define BF_DAS_BURST_TERM_H

#include "das_general.h"

constexpr int FB = (int)BF_BURST_FRAMES_PER_THREAD;

/* a term's weight in frame slot f: one apodization for every slot (RCA: float), or one per slot (READI: SlotWeights) */
struct SlotWeights { float w[FB]; };
__device__ __forceinline__ float slot_weight(float w, int) { return w; }
__device__ __forceinline__ float slot_weight(const SlotWeights &w, int f) { return w.w[f]; }

/* The frames of this block (grid y: groups of FB frames): first .. first + count - 1; the last group may hold fewer than FB. */
__device__ __forceinline__ void burst_frames(uint32_t frame_count, uint32_t &first, uint32_t &count)
{
	first = blockIdx.y * (uint32_t)FB;
	count = frame_count - first < (uint32_t)FB ? frame_count - first : (uint32_t)FB;
}

/* One in-aperture term of FB frames: sample_rf (das_common.h, das.glsl:99-124 + cubic :67-97) with everything that depends on the
 * index alone -- range test, tap, weights, phasor -- taken once.  A term outside the valid range adds nothing (sample_rf gives +0).
 * W: float, or SlotWeights (slot_weight). */
template <int INTERP, bool CPLX, bool CW, typename W>
__device__ __forceinline__ void burst_term(const char *const (&rf)[FB], int rf_offset, float index, W weights, const BfDasArgs &p,
                                           Accumulator<CPLX, CW, false> (&acc)[FB])
{
	/* The four frame slots must be the SAME arithmetic, so that a frame's bits do not depend on its place in the burst: left to itself
	 * hipcc fuses the multiply-adds of the unrolled slots independently (it did: one ulp between slots, real samples with coherency
	 * weighting).  Contraction is therefore off in here and every fused multiply-add is written out. */
	#pragma clang fp contract(off)
	constexpr uint32_t ES = CPLX ? 8 : 4;
	const float S = (float)p.sample_count;
	float c = 1.f, s = 0.f;
	auto phasor = [&]() {                                   /* rotate_iq's, das.glsl:54-61 */
		if constexpr (CPLX) {
			float turns = hw_fract(index * p.turns_per_sample);
			c = hw_cos_turns(turns); s = hw_sin_turns(turns);
		}
	};
	/* rotate, weight, RESULT_STORE (das.glsl:28-32) */
	auto add = [&](int f, sample_t<CPLX> v) {
		#pragma clang fp contract(off)
		const float apodization = slot_weight(weights, f);
		if constexpr (CPLX) {
			v = f32x2{__builtin_fmaf(c, v.x, -(s * v.y)), __builtin_fmaf(s, v.x, c * v.y)};
			if constexpr (CW) {
				const f32x2 w = apodization * v;
				acc[f].coherent += w;
				acc[f].incoherent += hw_sqrt(__builtin_fmaf(w.x, w.x, w.y * w.y));
			} else {
				acc[f].coherent = f32x2{__builtin_fmaf(apodization, v.x, acc[f].coherent.x), __builtin_fmaf(apodization, v.y, acc[f].coherent.y)};
			}
		} else {
			if constexpr (CW) {
				const float w = apodization * v;
				acc[f].coherent += w;
				acc[f].incoherent += __builtin_fabsf(w);
			} else {
				acc[f].coherent = __builtin_fmaf(apodization, v, acc[f].coherent);
			}
		}
	};
	auto fma2 = [](float a, f32x2 b, f32x2 c2) { return f32x2{__builtin_fmaf(a, b.x, c2.x), __builtin_fmaf(a, b.y, c2.y)}; };
	if constexpr (INTERP == BF_INTERP_NEAREST) {
		if (index >= 0.f && index < S - 0.5f) {
			int k = (int)__builtin_roundf(index);
			const uint32_t off = (uint32_t)(rf_offset + k) * ES;
			phasor();
			sample_t<CPLX> v[FB];
			for (int f = 0; f < FB; f++) v[f] = gather<sample_t<CPLX>>(rf[f], off);
			for (int f = 0; f < FB; f++) add(f, v[f]);
		}
	} else if constexpr (INTERP == BF_INTERP_LINEAR) {
		uint32_t k = (uint32_t)cvt_floor_i32(index);
		if (k < (uint32_t)(p.sample_count - 1)) {
			float t = hw_fract(index);
			const uint32_t off = ((uint32_t)rf_offset + k) * ES;
			phasor();
			if constexpr (CPLX) {
				f32x4 v[FB];
				for (int f = 0; f < FB; f++) v[f] = gather<f32x4_a8>(rf[f], off);
				for (int f = 0; f < FB; f++) {
					f32x2 a = {v[f].x, v[f].y}, b = {v[f].z, v[f].w};
					add(f, fma2(t, b - a, a));
				}
			} else {
				f32x2 v[FB];
				for (int f = 0; f < FB; f++) v[f] = gather<f32x2_a4>(rf[f], off);
				for (int f = 0; f < FB; f++) add(f, __builtin_fmaf(t, v[f].y - v[f].x, v[f].x));
			}
		}
	} else {
		uint32_t k = (uint32_t)(cvt_floor_i32(index) - 1);
		if (k < (uint32_t)(p.sample_count - 3)) {
			float t = hw_fract(index);
			const uint32_t off = ((uint32_t)rf_offset + k) * ES;
			float t2 = t * t, t3 = t2 * t;
			/* Hermite basis with tangents 0.5 (P2 - P0), 0.5 (P3 - P1) */
			float b0 =  2.f * t3 - 3.f * t2 + 1.f;
			float b1 = -2.f * t3 + 3.f * t2;
			float b2 =        t3 - 2.f * t2 + t;
			float b3 =        t3 -       t2;
			phasor();
			if constexpr (CPLX) {
				f32x4 lo[FB], hi[FB];
				for (int f = 0; f < FB; f++) { lo[f] = gather<f32x4_a8>(rf[f], off); hi[f] = gather<f32x4_a8>(rf[f], off + 16); }
				for (int f = 0; f < FB; f++) {
					f32x2 s0 = {lo[f].x, lo[f].y}, s1 = {lo[f].z, lo[f].w}, s2 = {hi[f].x, hi[f].y}, s3 = {hi[f].z, hi[f].w};
					f32x2 T1 = 0.5f * (s2 - s0), T2 = 0.5f * (s3 - s1);
					add(f, fma2(b3, T2, fma2(b2, T1, fma2(b1, s2, b0 * s1))));
				}
			} else {
				f32x4 v[FB];
				for (int f = 0; f < FB; f++) v[f] = gather<f32x4_a4>(rf[f], off);
				for (int f = 0; f < FB; f++) {
					float T1 = 0.5f * (v[f].z - v[f].x), T2 = 0.5f * (v[f].w - v[f].y);
					add(f, __builtin_fmaf(b3, T2, __builtin_fmaf(b2, T1, __builtin_fmaf(b1, v[f].z, b0 * v[f].y))));
				}
			}
		}
	}
}

#endif
