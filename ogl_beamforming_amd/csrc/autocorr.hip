/* autocorr.hip -- the slow-time autocorrelation of an ensemble on the frames of the frame ring (beamformer_hip_autocorrelate_last_frames):
 * the per-voxel reduction across slow time behind the ensemble filter of ensemble.hip.  include/ogl_beamformer_hip.h has the definition
 * for callers; tests/autocorr_ref.py restates it in numpy.
 *
 * AUTOCORRELATE.  y_n[v] = sum_k W[n][k] f_k[v], n = 0 .. rows - 1, each float the float32 fmaf chain of MIX (ensemble.hip): bit for
 * bit what beamformer_hip_mix_last_frames would have stored.  R_L[v] = sum over n = 0 .. rows - 1 - L of conj(y_n[v]) y_{n+L}[v] for
 * L = 0 .. lag_count - 1, each float one float32 fmaf chain from +0 in ascending n -- real part: fmaf(yr_n, yr_{n+L}, acc) then
 * fmaf(yi_n, yi_{n+L}, acc); imaginary part: fmaf(yr_n, yi_{n+L}, acc) then fmaf(-yi_n, yr_{n+L}, acc); real frames:
 * fmaf(y_n, y_{n+L}, acc) --, and the imaginary part of lag 0 is 0 * re(R_0): +0 where that real part is finite, NaN where it is not.
 *
 * A lane owns one voxel (consecutive lanes consecutive voxels: 8-byte accesses, 4-byte for real frames) and ALL rows; a block 256
 * voxels.  The rows are walked in tiles of BF_MIX_TILE: the 16 y values of a tile are formed as mix_kernel forms them (mix_term.h:
 * one text for both) -- 2 x 16 accumulator VGPRs, one load a source frame a lane, the tile's 32 weights of a source frame through
 * scalar loads from the table the host lays out [tile][k][16][2], so that the inner loop is fma with a scalar operand --, then row
 * m = 16 tile + j extends chain L with the term n = m - L: ascending m is ascending n.  y_{m-L} is a register of this tile (j >= L) or one of the
 * BEAMFORMER_HIP_MAX_LAGS - 1 = 3 newest y of the previous tile, carried across the boundary.  Every index into yr / yi / the carry /
 * the chains is a constant once the loops over j and L are unrolled: nothing goes to scratch.  The source loads run four frames
 * ahead of the fma that use them (a tile's 64 v_fma a source frame are ~256 cycles: four loads in flight cover an L2 hit).  The
 * ceil(rows / 16) reads of a source voxel after the first are served by L2 / Infinity Cache, as in the mix.  Rows past `rows` in the
 * last tile (zero rows of the weight table) and terms with n < 0 take no part in any chain: conditions that are uniform across the
 * block.  No LDS, no atomics.
 *
 * The identity form (weights == NULL: y_n = f_n, rows == K) is an instantiation of its own: a tile is 16 loads, each source read once. */
#include <hip/hip_runtime.h>
#include "bf_kernels.h"
#include "mix_term.h"

namespace {

constexpr uint32_t kCarry = BF_AUTOCORR_MAX_LAGS - 1u;    /* y values of the previous tile a chain can reach */
constexpr uint32_t kAhead = 4u;                           /* source frames loaded ahead of their fma */

template <bool CPLX>
__device__ __forceinline__ f32x2 voxel_of(const char *frame, uint64_t e)
{
	if (CPLX) return ((const f32x2 *)frame)[e];
	f32x2 r; r.x = ((const float *)frame)[e]; r.y = 0.0f;
	return r;
}

} // namespace

template <uint32_t LAGS, bool CPLX, bool IDENTITY>
__global__ __launch_bounds__(256) void autocorr_kernel(char *ring, const uint64_t *__restrict__ offsets, const float *__restrict__ weights,
                                                       BfAutocorrArgs a)
{
	static_assert(LAGS >= 1 && LAGS <= BF_AUTOCORR_MAX_LAGS && BF_AUTOCORR_MAX_LAGS <= BF_MIX_TILE, "a chain reaches one tile back at most");
	const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	if (e >= a.elements) return;
	float ar[LAGS], ai[LAGS];                                 /* the chains (ai[0] stays unused: lag 0's imaginary part is not a chain) */
	float pr[kCarry], pi[kCarry];                             /* y of rows first - 3, first - 2, first - 1 */
	#pragma unroll
	for (uint32_t l = 0; l < LAGS; l++) { ar[l] = 0.0f; ai[l] = 0.0f; }
	#pragma unroll
	for (uint32_t q = 0; q < kCarry; q++) { pr[q] = 0.0f; pi[q] = 0.0f; }

	const uint32_t last = a.frames - 1u;
	for (uint32_t first = 0; first < a.rows; first += BF_MIX_TILE) {
		float yr[BF_MIX_TILE], yi[BF_MIX_TILE];
		if (IDENTITY) {
			/* rows == frames: row m is frame m (past the last one: the last one again, which no chain takes) */
			#pragma unroll
			for (uint32_t j = 0; j < BF_MIX_TILE; j++) {
				const uint32_t m = first + j;
				const f32x2 c = voxel_of<CPLX>(ring + offsets[m < last ? m : last], e);
				yr[j] = c.x; yi[j] = c.y;
			}
		} else {
			const float *w = weights + (uint64_t)(first / BF_MIX_TILE) * a.frames * (2u * BF_MIX_TILE);
			#pragma unroll
			for (uint32_t j = 0; j < BF_MIX_TILE; j++) { yr[j] = 0.0f; yi[j] = 0.0f; }
			f32x2 cur[kAhead], next[kAhead];
			#pragma unroll
			for (uint32_t q = 0; q < kAhead; q++) cur[q] = voxel_of<CPLX>(ring + offsets[q < last ? q : last], e);
			uint32_t k0 = 0;
			for (; k0 + kAhead <= a.frames; k0 += kAhead) {       /* whole groups: one basic block, the next group's loads in flight */
				#pragma unroll
				for (uint32_t q = 0; q < kAhead; q++) {
					const uint32_t k = k0 + kAhead + q;
					next[q] = voxel_of<CPLX>(ring + offsets[k < last ? k : last], e);
				}
				__builtin_amdgcn_sched_barrier(0);                /* (the scheduler would sink these loads to the end of the block, in front of their use) */
				#pragma unroll
				for (uint32_t q = 0; q < kAhead; q++, w += 2u * BF_MIX_TILE) mix_term<CPLX>(yr, yi, cur[q], w);
				#pragma unroll
				for (uint32_t q = 0; q < kAhead; q++) cur[q] = next[q];
			}
			#pragma unroll
			for (uint32_t q = 0; q + 1u < kAhead; q++)            /* the frames past the last whole group */
				if (k0 + q < a.frames) { mix_term<CPLX>(yr, yi, cur[q], w); w += 2u * BF_MIX_TILE; }
		}

		#pragma unroll
		for (uint32_t j = 0; j < BF_MIX_TILE; j++) {
			if (first + j < a.rows) {
				#pragma unroll
				for (uint32_t l = 0; l < LAGS; l++) {
					const bool here = j >= l;                     /* y_{m-l} is a row of this tile; else, in the first tile, n = m - l < 0: no such term */
					if (here || first != 0) {
						const float br = here ? yr[here ? j - l : 0u] : pr[here ? 0u : kCarry + j - l];
						const float bi = here ? yi[here ? j - l : 0u] : pi[here ? 0u : kCarry + j - l];
						ar[l] = __builtin_fmaf(br, yr[j], ar[l]);
						if (CPLX) {
							ar[l] = __builtin_fmaf(bi, yi[j], ar[l]);
							if (l) { ai[l] = __builtin_fmaf(br, yi[j], ai[l]); ai[l] = __builtin_fmaf(-bi, yr[j], ai[l]); }
						}
					}
				}
			}
		}
		#pragma unroll
		for (uint32_t q = 0; q < kCarry; q++) { pr[q] = yr[BF_MIX_TILE - kCarry + q]; pi[q] = yi[BF_MIX_TILE - kCarry + q]; }
	}

	char *out = ring + a.out_offset;
	#pragma unroll
	for (uint32_t l = 0; l < LAGS; l++, out += a.out_stride) {
		if (CPLX) { f32x2 c; c.x = ar[l]; c.y = l ? ai[l] : ar[0] * 0.0f; ((f32x2 *)out)[e] = c; }
		else      ((float *)out)[e] = ar[l];
	}
}

namespace {

template <uint32_t LAGS>
hipError_t launch(void *ring, const uint64_t *offsets, const float *weights, const BfAutocorrArgs &a, uint32_t blocks, hipStream_t s)
{
	const dim3 grid(blocks), block(256);
	if (weights) {
		if (a.cplx) hipLaunchKernelGGL((autocorr_kernel<LAGS, true, false>), grid, block, 0, s, (char *)ring, offsets, weights, a);
		else        hipLaunchKernelGGL((autocorr_kernel<LAGS, false, false>), grid, block, 0, s, (char *)ring, offsets, weights, a);
	} else {
		if (a.cplx) hipLaunchKernelGGL((autocorr_kernel<LAGS, true, true>), grid, block, 0, s, (char *)ring, offsets, weights, a);
		else        hipLaunchKernelGGL((autocorr_kernel<LAGS, false, true>), grid, block, 0, s, (char *)ring, offsets, weights, a);
	}
	return hipGetLastError();
}

} // namespace

/* Every table is device memory.  Every frame and the output run lie inside the ring, and the output run clear of the source frames:
 * the caller's business (frame_ops.cpp: autocorrelate_last_frames), nothing here re-checks it. */
extern "C" hipError_t bf_launch_autocorr(void *ring, const uint64_t *offsets, const float *weights, const BfAutocorrArgs *a, hipStream_t s)
{
	if (!ring || !offsets || !a || a->frames == 0 || a->frames > BF_ENSEMBLE_MAX_FRAMES || a->rows == 0 || a->rows > BF_ENSEMBLE_MAX_FRAMES ||
	    a->lags == 0 || a->lags > BF_AUTOCORR_MAX_LAGS || a->lags > a->rows || (!weights && a->rows != a->frames) || a->elements == 0)
		return hipErrorInvalidValue;
	const uint64_t blocks = (a->elements + 255u) / 256u;
	if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
	switch (a->lags) {
	case 1:  return launch<1>(ring, offsets, weights, *a, (uint32_t)blocks, s);
	case 2:  return launch<2>(ring, offsets, weights, *a, (uint32_t)blocks, s);
	case 3:  return launch<3>(ring, offsets, weights, *a, (uint32_t)blocks, s);
	default: return launch<4>(ring, offsets, weights, *a, (uint32_t)blocks, s);
	}
}
