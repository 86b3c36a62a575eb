/* mix_term.h -- one source frame's term of the MIX chains (include/ogl_beamformer_hip.h), shared by the two kernels that form them:
 * mix_kernel (ensemble.hip), which stores the sums, and autocorr_kernel (autocorr.hip), which reduces them further -- one text, so
 * that the filtered samples of the second are the frames of the first bit for bit. */
#ifndef BF_MIX_TERM_H
#define BF_MIX_TERM_H
#include "bf_kernels.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

/* re[j] / im[j]: the chains of the tile's BF_MIX_TILE outputs; c: the source voxel (real frames: c.x); w[BF_MIX_TILE][2]: the tile's
 * weights of this source frame, uniform across the block (real frames: the imaginary ones are not read, im is not touched) */
template <bool CPLX>
__device__ __forceinline__ void mix_term(float (&re)[BF_MIX_TILE], float (&im)[BF_MIX_TILE], f32x2 c, const float *__restrict__ w)
{
	#pragma unroll
	for (uint32_t j = 0; j < BF_MIX_TILE; j++) {
		const float wr = w[2u * j], wi = w[2u * j + 1u];
		if (CPLX) {
			re[j] = __builtin_fmaf(wr, c.x, re[j]); re[j] = __builtin_fmaf(-wi, c.y, re[j]);
			im[j] = __builtin_fmaf(wi, c.x, im[j]); im[j] = __builtin_fmaf(wr, c.y, im[j]);
		} else {
			re[j] = __builtin_fmaf(wr, c.x, re[j]);
		}
	}
}
#endif
