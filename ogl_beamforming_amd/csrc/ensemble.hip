/* ensemble.hip -- the two slow-time primitives of the ensemble filter on the frames of the frame ring: the K x K Gram matrix of the K
 * newest frames (beamformer_hip_gram_last_frames) and M linear combinations of them written back as frames
 * (beamformer_hip_mix_last_frames).  include/ogl_beamformer_hip.h has the definitions for callers; tests/ensemble_ref.py restates them
 * in numpy.
 *
 * GRAM.  G[j][k] = sum over the box's voxels v that are finite in ALL K frames of conj(f_j[v]) * f_k[v].  Every float is widened to
 * double; the products of two widened floats are exact in double, so rj * rk + ij * ik and rj * ik - ij * rk are ONE rounding each
 * whether or not the second product is fused into the addition (it is written as an fma); adding a term to the running sum is one more.
 * Three launches, no atomics:
 *   mask     a wave owns one word: 64 consecutive voxels of the box in flat box order (x fastest).  A lane reads its voxel of every
 *            frame -- consecutive lanes consecutive voxels of a box row -- and a ballot makes the word: bit set = inside the box and
 *            finite in every frame.  (The mask is a pass of its own, not a step of the partial pass: from 33 frames on a block of the
 *            partial pass holds two tiles of 32 frames, not all K.)
 *   partial  grid x the chunk -- a run of whole words, bf_gram_chunk_words: a function of the box and K alone --, grid y the tile pair
 *            (tj <= tk) of 32 x 32 frame pairs.  Per word the block stages the 64 voxels of the (up to) 64 frames of its two tiles in
 *            LDS, [voxel][frame], a row 65 entries long: the staging stores of a wave (64 voxels of one frame) are 2-way on the
 *            banks, the reads of a voxel's row conflict-free.  Thread t owns the pairs (j = t / 8, k = 4 * (t % 8) .. + 3) of the tile
 *            pair and walks the word's set bits in ascending order with eight double accumulators; one double2 a pair a block.  A
 *            diagonal tile pair computes its lower triangle too (nobody reads it); frames past K are staged as zeros.
 *   fold     a thread a pair j <= k sums its chunks' partials in chunk order, stores G[j][k] and the exact conjugate at G[k][j]
 *            (0 - im: a zero stays +0) and 0 for a diagonal's imaginary part; one more block counts the mask's bits.
 * The order of every addition is fixed by the box and K: the bytes of a result repeat.
 *
 * MIX.  out_j[v] = sum_k W[j][k] * f_k[v] as float32 fmaf chains from +0 in ascending k -- real part: fmaf(Wre, re_k, acc) then
 * fmaf(-Wim, im_k, acc); imaginary part: fmaf(Wim, re_k, acc) then fmaf(Wre, im_k, acc) --, no weight skipped, nothing special-cased
 * for NaN.  A lane owns one voxel (consecutive lanes consecutive voxels: 8-byte accesses, 4-byte for real frames), a block 256 voxels
 * and a tile of BF_MIX_TILE output frames: 2 x 16 accumulator VGPRs.  Per source frame k: one load a lane, and the tile's 32 weights
 * -- uniform across the block, laid out [tile][k][16][2] by the host -- through scalar loads, so that the inner loop is v_fma_f32 with
 * a scalar operand.  Blocks of one voxel range and different output tiles are neighbours in the grid: the ceil(M / 16) reads of a
 * source voxel after the first are served by L2 / Infinity Cache.  Tails are bounds: lanes past the frame's last voxel leave at once,
 * output rows past M (zero rows of the weight table) are not stored. */
#include <hip/hip_runtime.h>
#include "bf_kernels.h"
#include "gram_body.h"

/* the three passes of one box: their bodies are gram_body.h's, which ensemble_blocks.hip runs over many boxes a launch */
__global__ __launch_bounds__(256) void gram_mask_kernel(const char *__restrict__ ring, const uint64_t *__restrict__ offsets, BfGramArgs a,
                                                        uint64_t *__restrict__ mask)
{
	gram_mask_body(ring, offsets, a, blockIdx.x, mask);
}

__global__ __launch_bounds__(256) void gram_partial_kernel(const char *__restrict__ ring, const uint64_t *__restrict__ offsets, BfGramArgs a,
                                                           const uint64_t *__restrict__ mask, double2 *__restrict__ partials)
{
	__shared__ f32x2 tile[BF_GRAM_WORD * kGramRow];           /* [voxel][slot]: slots 0 .. 31 the frames of tile tj, 32 .. 63 those of tile tk */
	gram_partial_body(ring, offsets, a, blockIdx.x, blockIdx.y, tile, mask, partials);
}

/* grid y: the frame j, and one more row whose first block counts the mask; grid x: 64 frames k a block */
__global__ __launch_bounds__(64) void gram_fold_kernel(BfGramArgs a, const uint64_t *__restrict__ mask, const double2 *__restrict__ partials,
                                                       uint64_t *__restrict__ counts, double2 *__restrict__ gram)
{
	gram_fold_body(a, blockIdx.x, blockIdx.y, mask, partials, counts, gram);
}

template <bool CPLX>
__global__ __launch_bounds__(256) void mix_kernel(char *ring, const uint64_t *__restrict__ offsets, const float *__restrict__ weights, BfMixArgs a)
{
	const uint32_t tiles = a.padded_outputs / BF_MIX_TILE;
	const uint32_t tile = blockIdx.x % tiles;
	const uint64_t e = (uint64_t)(blockIdx.x / tiles) * 256u + threadIdx.x;
	if (e >= a.elements) return;
	const float *w = weights + (uint64_t)tile * a.frames * (2u * BF_MIX_TILE);
	float re[BF_MIX_TILE], im[BF_MIX_TILE];
	#pragma unroll
	for (uint32_t j = 0; j < BF_MIX_TILE; j++) { re[j] = 0.0f; im[j] = 0.0f; }
	for (uint32_t k = 0; k < a.frames; k++, w += 2u * BF_MIX_TILE) {
		const char *frame = ring + offsets[k];
		f32x2 c;
		if (CPLX) c = ((const f32x2 *)frame)[e];
		else      { c.x = ((const float *)frame)[e]; c.y = 0.0f; }
		mix_term<CPLX>(re, im, c, w);
	}
	char *out = ring + a.out_offset + (uint64_t)tile * BF_MIX_TILE * a.out_stride;
	#pragma unroll
	for (uint32_t j = 0; j < BF_MIX_TILE; j++, out += a.out_stride) {
		if (tile * BF_MIX_TILE + j >= a.outputs) break;
		if (CPLX) { f32x2 c; c.x = re[j]; c.y = im[j]; ((f32x2 *)out)[e] = c; }
		else      ((float *)out)[e] = re[j];
	}
}

/* Every table is device memory.  The box lies inside every frame, every frame and the output run inside the ring, and the output run
 * clear of the source frames: the caller's business (frame_ops.cpp: gram_last_frames, mix_last_frames), nothing here re-checks it. */
extern "C" hipError_t bf_launch_gram(const void *ring, const uint64_t *offsets, const BfGramArgs *a, uint64_t *mask, double *partials, void *result,
                                     hipStream_t s)
{
	if (!ring || !offsets || !a || !mask || !partials || !result || a->frames == 0 || a->frames > BF_ENSEMBLE_MAX_FRAMES || a->volume == 0 ||
	    a->words != (uint32_t)(((uint64_t)a->volume + BF_GRAM_WORD - 1u) / BF_GRAM_WORD) || a->chunk_words == 0 ||
	    a->chunks != (a->words + a->chunk_words - 1u) / a->chunk_words || a->tiles != bf_gram_tiles(a->frames) ||
	    a->tile_pairs != bf_gram_tile_pairs(a->frames))
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(gram_mask_kernel, dim3((a->words + 3u) / 4u), dim3(256), 0, s, (const char *)ring, offsets, *a, mask);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(gram_partial_kernel, dim3(a->chunks, a->tile_pairs), dim3(256), 0, s, (const char *)ring, offsets, *a, (const uint64_t *)mask,
	                   (double2 *)partials);
	e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(gram_fold_kernel, dim3((a->frames + 63u) / 64u, a->frames + 1u), dim3(64), 0, s, *a, (const uint64_t *)mask,
	                   (const double2 *)partials, (uint64_t *)result, (double2 *)((char *)result + 16));
	return hipGetLastError();
}

extern "C" hipError_t bf_launch_mix(void *ring, const uint64_t *offsets, const float *weights, const BfMixArgs *a, hipStream_t s)
{
	if (!ring || !offsets || !weights || !a || a->frames == 0 || a->frames > BF_ENSEMBLE_MAX_FRAMES || a->outputs == 0 ||
	    a->outputs > BF_ENSEMBLE_MAX_FRAMES || a->padded_outputs != (a->outputs + BF_MIX_TILE - 1u) / BF_MIX_TILE * BF_MIX_TILE || a->elements == 0)
		return hipErrorInvalidValue;
	const uint64_t blocks = (a->elements + 255u) / 256u * (a->padded_outputs / BF_MIX_TILE);
	if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
	if (a->cplx) hipLaunchKernelGGL(mix_kernel<true>, dim3((uint32_t)blocks), dim3(256), 0, s, (char *)ring, offsets, weights, *a);
	else         hipLaunchKernelGGL(mix_kernel<false>, dim3((uint32_t)blocks), dim3(256), 0, s, (char *)ring, offsets, weights, *a);
	return hipGetLastError();
}
