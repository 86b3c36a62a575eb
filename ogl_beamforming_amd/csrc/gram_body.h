/* gram_body.h -- one box's share of the three passes of the Gram matrix (include/ogl_beamformer_hip.h: GRAM), shared by the kernels that
 * run them: gram_mask_kernel, gram_partial_kernel and gram_fold_kernel (ensemble.hip), one box a launch, and blocks_mask_kernel,
 * blocks_partial_kernel and blocks_fold_kernel (ensemble_blocks.hip), many boxes a launch -- one text, so that the matrix of a box of
 * the second is the matrix of the first bit for bit.  A body is handed the box's arguments, the block's place INSIDE the box (what
 * blockIdx is in the single-box launch) and the box's own mask, partials and result; ensemble.hip describes the passes. */
#ifndef BF_GRAM_BODY_H
#define BF_GRAM_BODY_H
#include "mix_term.h"

constexpr uint32_t kGramRow = BF_GRAM_WORD + 1u;      /* an LDS row: 64 frame slots and one of padding */

__device__ __forceinline__ bool gram_is_finite(float a) { return (__float_as_uint(a) & 0x7F800000u) != 0x7F800000u; }

/* voxel v of the box (flat, x fastest) as a flat index in the frame */
__device__ __forceinline__ uint64_t gram_frame_index(const BfGramArgs &a, uint32_t v)
{
	const uint32_t rest = v / a.count[0], x = v - rest * a.count[0], z = rest / a.count[1], y = rest - z * a.count[1];
	return ((uint64_t)(z + a.first[2]) * a.points[1] + (y + a.first[1])) * a.points[0] + (x + a.first[0]);
}

__device__ __forceinline__ f32x2 gram_voxel_at(const char *frame, uint64_t i, uint32_t cplx)
{
	if (cplx) return ((const f32x2 *)frame)[i];
	f32x2 r; r.x = ((const float *)frame)[i]; r.y = 0.0f;
	return r;
}

/* block: the box's block of the mask pass, 256 threads, a wave a word */
__device__ __forceinline__ void gram_mask_body(const char *__restrict__ ring, const uint64_t *__restrict__ offsets, const BfGramArgs &a,
                                               uint32_t block, uint64_t *__restrict__ mask)
{
	const uint32_t word = block * 4u + (threadIdx.x >> 6);
	if (word >= a.words) return;                              /* (a whole wave: the ballot below sees all 64 lanes or none) */
	const uint32_t v = word * BF_GRAM_WORD + (threadIdx.x & 63u);
	bool good = v < a.volume;                                 /* (the volume is below 2^32: word * 64 <= 2^32 - 64 does not wrap) */
	if (good) {
		const uint64_t i = gram_frame_index(a, v);
		for (uint32_t k = 0; k < a.frames; k++) {
			const f32x2 c = gram_voxel_at(ring + offsets[k], i, a.cplx);
			good = good && gram_is_finite(c.x) && gram_is_finite(c.y);
		}
	}
	const uint64_t bits = __ballot(good);
	if ((threadIdx.x & 63u) == 0) mask[word] = bits;
}

/* chunk, pair: the box's block of the partial pass, 256 threads; tile: BF_GRAM_WORD * kGramRow entries of LDS, [voxel][slot] -- slots
 * 0 .. 31 the frames of tile tj, 32 .. 63 those of tile tk */
__device__ __forceinline__ void gram_partial_body(const char *__restrict__ ring, const uint64_t *__restrict__ offsets, const BfGramArgs &a,
                                                  uint32_t chunk, uint32_t pair, f32x2 *tile, const uint64_t *__restrict__ mask,
                                                  double2 *__restrict__ partials)
{
	#pragma clang fp contract(off)
	/* the tile pair, row by row through the upper triangle */
	uint32_t tj = 0, rest = pair;
	while (rest >= a.tiles - tj) { rest -= a.tiles - tj; tj++; }
	const uint32_t tk = tj + rest;
	const uint32_t slots = tj == tk ? BF_GRAM_TILE : 2u * BF_GRAM_TILE, k_slot0 = tj == tk ? 0u : BF_GRAM_TILE;

	const uint32_t lane_voxel = threadIdx.x & 63u, slot0 = threadIdx.x >> 6;
	const uint32_t jj = threadIdx.x >> 3, kq = (threadIdx.x & 7u) * 4u;

	double re[4] = {0.0, 0.0, 0.0, 0.0}, im[4] = {0.0, 0.0, 0.0, 0.0};
	const uint32_t word_first = chunk * a.chunk_words;
	const uint32_t word_end = word_first + a.chunk_words < a.words ? word_first + a.chunk_words : a.words;
	for (uint32_t word = word_first; word < word_end; word++) {
		const uint32_t v = word * BF_GRAM_WORD + lane_voxel;
		const bool inside = v < a.volume;
		const uint64_t i = inside ? gram_frame_index(a, v) : 0;
		for (uint32_t slot = slot0; slot < slots; slot += 4u) {
			const uint32_t frame = slot < BF_GRAM_TILE ? tj * BF_GRAM_TILE + slot : tk * BF_GRAM_TILE + (slot - BF_GRAM_TILE);
			f32x2 c; c.x = 0.0f; c.y = 0.0f;
			if (inside && frame < a.frames) c = gram_voxel_at(ring + offsets[frame], i, a.cplx);
			tile[lane_voxel * kGramRow + slot] = c;
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
			const f32x2 *row = tile + n * kGramRow;
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
	double2 *out = partials + ((uint64_t)chunk * a.tile_pairs + pair) * (BF_GRAM_TILE * BF_GRAM_TILE) + jj * BF_GRAM_TILE + kq;
	#pragma unroll
	for (uint32_t q = 0; q < 4u; q++) { double2 p; p.x = re[q]; p.y = im[q]; out[q] = p; }
}

/* j: the frame j, or a.frames: the row whose first block counts the mask; block: 64 frames k a block, 64 threads */
__device__ __forceinline__ void gram_fold_body(const BfGramArgs &a, uint32_t block, uint32_t j, const uint64_t *__restrict__ mask,
                                               const double2 *__restrict__ partials, uint64_t *__restrict__ counts, double2 *__restrict__ gram)
{
	#pragma clang fp contract(off)
	if (j == a.frames) {
		if (block) return;
		uint64_t good = 0;
		for (uint32_t word = threadIdx.x; word < a.words; word += 64u) good += (uint64_t)__popcll(mask[word]);
		for (int off = 32; off > 0; off >>= 1) good += __shfl_xor((unsigned long long)good, off, 64);
		if (threadIdx.x == 0) { counts[0] = good; counts[1] = (uint64_t)a.volume - good; }
		return;
	}
	const uint32_t k = block * 64u + threadIdx.x;
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
#endif
