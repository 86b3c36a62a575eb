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
#include "mix_term.h"

namespace {

constexpr uint32_t kRow = BF_GRAM_WORD + 1u;          /* an LDS row: 64 frame slots and one of padding */

__device__ __forceinline__ bool is_finite(float a) { return (__float_as_uint(a) & 0x7F800000u) != 0x7F800000u; }

/* voxel v of the box (flat, x fastest) as a flat index in the frame */
__device__ __forceinline__ uint64_t frame_index(const BfGramArgs &a, uint32_t v)
{
	const uint32_t rest = v / a.count[0], x = v - rest * a.count[0], z = rest / a.count[1], y = rest - z * a.count[1];
	return ((uint64_t)(z + a.first[2]) * a.points[1] + (y + a.first[1])) * a.points[0] + (x + a.first[0]);
}

__device__ __forceinline__ f32x2 voxel_at(const char *frame, uint64_t i, uint32_t cplx)
{
	if (cplx) return ((const f32x2 *)frame)[i];
	f32x2 r; r.x = ((const float *)frame)[i]; r.y = 0.0f;
	return r;
}

} // namespace

__global__ __launch_bounds__(256) void gram_mask_kernel(const char *__restrict__ ring, const uint64_t *__restrict__ offsets, BfGramArgs a,
                                                        uint64_t *__restrict__ mask)
{
	const uint32_t word = blockIdx.x * 4u + (threadIdx.x >> 6);
	if (word >= a.words) return;                              /* (a whole wave: the ballot below sees all 64 lanes or none) */
	const uint32_t v = word * BF_GRAM_WORD + (threadIdx.x & 63u);
	bool good = v < a.volume;                                 /* (the volume is below 2^32: word * 64 <= 2^32 - 64 does not wrap) */
	if (good) {
		const uint64_t i = frame_index(a, v);
		for (uint32_t k = 0; k < a.frames; k++) {
			const f32x2 c = voxel_at(ring + offsets[k], i, a.cplx);
			good = good && is_finite(c.x) && is_finite(c.y);
		}
	}
	const uint64_t bits = __ballot(good);
	if ((threadIdx.x & 63u) == 0) mask[word] = bits;
}

__global__ __launch_bounds__(256) void gram_partial_kernel(const char *__restrict__ ring, const uint64_t *__restrict__ offsets, BfGramArgs a,
                                                           const uint64_t *__restrict__ mask, double2 *__restrict__ partials)
{
	#pragma clang fp contract(off)
	__shared__ f32x2 tile[BF_GRAM_WORD * kRow];               /* [voxel][slot]: slots 0 .. 31 the frames of tile tj, 32 .. 63 those of tile tk */

	/* the tile pair, row by row through the upper triangle */
	uint32_t tj = 0, rest = blockIdx.y;
	while (rest >= a.tiles - tj) { rest -= a.tiles - tj; tj++; }
	const uint32_t tk = tj + rest;
	const uint32_t slots = tj == tk ? BF_GRAM_TILE : 2u * BF_GRAM_TILE, k_slot0 = tj == tk ? 0u : BF_GRAM_TILE;

	const uint32_t lane_voxel = threadIdx.x & 63u, slot0 = threadIdx.x >> 6;
	const uint32_t jj = threadIdx.x >> 3, kq = (threadIdx.x & 7u) * 4u;

	double re[4] = {0.0, 0.0, 0.0, 0.0}, im[4] = {0.0, 0.0, 0.0, 0.0};
	const uint32_t word_first = blockIdx.x * a.chunk_words;
	const uint32_t word_end = word_first + a.chunk_words < a.words ? word_first + a.chunk_words : a.words;
	for (uint32_t word = word_first; word < word_end; word++) {
		const uint32_t v = word * BF_GRAM_WORD + lane_voxel;
		const bool inside = v < a.volume;
		const uint64_t i = inside ? frame_index(a, v) : 0;
		for (uint32_t slot = slot0; slot < slots; slot += 4u) {
			const uint32_t frame = slot < BF_GRAM_TILE ? tj * BF_GRAM_TILE + slot : tk * BF_GRAM_TILE + (slot - BF_GRAM_TILE);
			f32x2 c; c.x = 0.0f; c.y = 0.0f;
			if (inside && frame < a.frames) c = voxel_at(ring + offsets[frame], i, a.cplx);
			tile[lane_voxel * kRow + slot] = c;
		}
		__syncthreads();
		const uint64_t word_bits = mask[word];
		/* (uniform by construction; readfirstlane returns an int: through uint32_t, or a set bit 31 of the low half would extend over the high one) */
		const uint32_t bits_low  = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)word_bits);
		const uint32_t bits_high = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(word_bits >> 32));
		uint64_t bits = ((uint64_t)bits_high << 32) | (uint64_t)bits_low;
		while (bits) {                                        /* the word's voxels that count, in ascending order */
			const uint32_t n = (uint32_t)__builtin_ctzll(bits);
			bits &= bits - 1u;
			const f32x2 *row = tile + n * kRow;
			const f32x2 fj = row[jj];
			const double rj = (double)fj.x, ij = (double)fj.y;
			#pragma unroll
			for (uint32_t q = 0; q < 4u; q++) {
				const f32x2 fk = row[k_slot0 + kq + q];
				const double rk = (double)fk.x, ik = (double)fk.y;
				re[q] = re[q] + __builtin_fma(ij, ik, rj * rk);
				im[q] = im[q] + __builtin_fma(-ij, rk, rj * ik);
			}
		}
		__syncthreads();
	}
	double2 *out = partials + ((uint64_t)blockIdx.x * a.tile_pairs + blockIdx.y) * (BF_GRAM_TILE * BF_GRAM_TILE) + jj * BF_GRAM_TILE + kq;
	#pragma unroll
	for (uint32_t q = 0; q < 4u; q++) { double2 p; p.x = re[q]; p.y = im[q]; out[q] = p; }
}

/* grid y: the frame j, and one more row whose first block counts the mask; grid x: 64 frames k a block */
__global__ __launch_bounds__(64) void gram_fold_kernel(BfGramArgs a, const uint64_t *__restrict__ mask, const double2 *__restrict__ partials,
                                                       uint64_t *__restrict__ counts, double2 *__restrict__ gram)
{
	#pragma clang fp contract(off)
	if (blockIdx.y == a.frames) {
		if (blockIdx.x) return;
		uint64_t good = 0;
		for (uint32_t word = threadIdx.x; word < a.words; word += 64u) good += (uint64_t)__popcll(mask[word]);
		for (int off = 32; off > 0; off >>= 1) good += __shfl_xor((unsigned long long)good, off, 64);
		if (threadIdx.x == 0) { counts[0] = good; counts[1] = (uint64_t)a.volume - good; }
		return;
	}
	const uint32_t j = blockIdx.y, k = blockIdx.x * 64u + threadIdx.x;
	if (k < j || k >= a.frames) return;
	const uint32_t tj = j / BF_GRAM_TILE, tk = k / BF_GRAM_TILE;
	const uint32_t pair = tj * a.tiles - tj * (tj - 1u) / 2u + (tk - tj);      /* (tj = 0: the product is 0 before the wrap matters) */
	const double2 *p = partials + (uint64_t)pair * (BF_GRAM_TILE * BF_GRAM_TILE) + (j % BF_GRAM_TILE) * BF_GRAM_TILE + k % BF_GRAM_TILE;
	const uint64_t step = (uint64_t)a.tile_pairs * (BF_GRAM_TILE * BF_GRAM_TILE);
	double re = 0.0, im = 0.0;
	for (uint32_t chunk = 0; chunk < a.chunks; chunk++, p += step) { const double2 t = *p; re = re + t.x; im = im + t.y; }
	if (j == k) im = 0.0;
	double2 upper, lower;
	upper.x = re; upper.y = im;
	lower.x = re; lower.y = 0.0 - im;
	gram[(uint64_t)j * a.frames + k] = upper;
	gram[(uint64_t)k * a.frames + j] = lower;
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
