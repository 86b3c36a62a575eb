/* ensemble_blocks.hip -- the block-wise form of the ensemble filter on the frames of the frame ring: the Gram matrices of many boxes in
 * one call (beamformer_hip_gram_boxes_last_frames) and a mix whose weight table varies over the frame, given at the nodes of a lattice
 * and blended between them (beamformer_hip_mix_field_last_frames).  include/ogl_beamformer_hip.h has the definitions for callers;
 * tests/block_filter_ref.py restates them in numpy.
 *
 * GRAM BOXES.  The matrix of a box is the single-box call's, bit for bit: the three passes of ensemble.hip run their bodies
 * (gram_body.h) with the box's own BfGramArgs -- its own chunking, bf_gram_chunk_words of its volume --, its own mask words and its own
 * partials.  A launch covers a BATCH of boxes: the device table BfBlocksBox holds, a box, the arguments, a prefix of block counts and
 * where the box's mask, partials and result lie.
 *   blocks_mask_kernel      a block finds its box by bisection over the prefix (its index is uniform: scalar loads), then is block
 *                           `index - prefix` of that box's mask pass
 *   blocks_partial_kernel   the same over the prefix of chunks x tile pairs; inside a box the tile pair runs fastest
 *   blocks_fold_kernel      grid z the box, grid x and y as gram_fold_kernel's
 * The host (frame_ops.cpp) walks the boxes in batches whose partials fit a budget; the batches sit behind one another on the stream and
 * reuse one mask and one partials buffer.
 *
 * FIELD MIX.  For node c the value y_c[j][v] is the MIX chain under W[c][j][.] -- mix_term.h, the text mix_kernel runs --; a voxel's
 * output is the lerp fmaf(t, b - a, a) of its corner nodes' values, along x, then y, then z.  The frame is cut into SEGMENT CELLS, the
 * product of one segment an axis (in front of the first node, between two neighbours, from the last node on): inside a cell the (up to)
 * 8 corner nodes are the same for every voxel, so a block that stays inside one cell has uniform weights -- scalar loads, v_fma_f32
 * with a scalar operand, as in mix_kernel -- and a voxel's r along an axis is its index inside the cell.
 *   blend_kernel<CPLX>      a block finds its cell by bisection over the cells' block prefix, then is (256-voxel tile of the cell's box,
 *                           x fastest; tile of BF_MIX_TILE outputs), the output tile fastest.  The corners run OUTERMOST, z, y, x with
 *                           x fastest: a corner's chains are formed over all K sources (2 x 16 accumulators), then folded into a
 *                           three-level stack -- the x pair is adjacent, so the lerp along x closes at every second corner, the one
 *                           along y at every fourth, the one along z at the eighth.  4 x 32 VGPRs of accumulators and stack.  The
 *                           sources are read once a corner; after the first they come from L2.
 * What bounds blend_kernel: a corner costs what a plain mix of the same K and M costs -- the same loads, the same FMAs --, so a cell
 * with C corners costs C plain mixes and the lerps (3 VALU operations an output float a closed level) on top; cells of few voxels add
 * idle lanes (a cell's last tile) and short rows (a cell's box is narrower than the frame, so a wave's 64 voxels span several rows).
 * Tails are bounds: lanes past the cell's last voxel leave at once, output rows past M (zero rows of the table) are not stored. */
#include <hip/hip_runtime.h>
#include "bf_kernels.h"
#include "gram_body.h"

namespace {

/* the last row whose prefix (member `first`) is <= block: rows[0]'s prefix is 0, `block` is uniform */
template <class Row>
__device__ __forceinline__ uint32_t row_of_block(const Row *__restrict__ rows, uint32_t count, uint32_t Row::*first, uint32_t block)
{
	uint32_t lo = 0, hi = count;
	while (hi - lo > 1u) {
		const uint32_t mid = lo + (hi - lo) / 2u;
		if (rows[mid].*first <= block) lo = mid; else hi = mid;
	}
	return lo;
}

} // namespace

__global__ __launch_bounds__(256) void blocks_mask_kernel(const char *__restrict__ ring, const uint64_t *__restrict__ offsets,
                                                          const BfBlocksBox *__restrict__ boxes, uint32_t box_count, uint64_t *__restrict__ mask)
{
	const uint32_t b = row_of_block(boxes, box_count, &BfBlocksBox::mask_block_first, blockIdx.x);
	const BfGramArgs a = boxes[b].a;
	gram_mask_body(ring, offsets, a, blockIdx.x - boxes[b].mask_block_first, mask + boxes[b].mask_first);
}

__global__ __launch_bounds__(256) void blocks_partial_kernel(const char *__restrict__ ring, const uint64_t *__restrict__ offsets,
                                                             const BfBlocksBox *__restrict__ boxes, uint32_t box_count,
                                                             const uint64_t *__restrict__ mask, double2 *__restrict__ partials)
{
	__shared__ f32x2 tile[BF_GRAM_WORD * kGramRow];
	const uint32_t b = row_of_block(boxes, box_count, &BfBlocksBox::partial_block_first, blockIdx.x);
	const BfGramArgs a = boxes[b].a;
	const uint32_t block = blockIdx.x - boxes[b].partial_block_first;
	gram_partial_body(ring, offsets, a, block / a.tile_pairs, block % a.tile_pairs, tile, mask + boxes[b].mask_first,
	                  partials + boxes[b].partial_first * (BF_GRAM_TILE * BF_GRAM_TILE));
}

__global__ __launch_bounds__(64) void blocks_fold_kernel(const BfBlocksBox *__restrict__ boxes, const uint64_t *__restrict__ mask,
                                                         const double2 *__restrict__ partials, char *__restrict__ results)
{
	const BfGramArgs a = boxes[blockIdx.z].a;
	char *result = results + boxes[blockIdx.z].result_first;
	gram_fold_body(a, blockIdx.x, blockIdx.y, mask + boxes[blockIdx.z].mask_first,
	               partials + boxes[blockIdx.z].partial_first * (BF_GRAM_TILE * BF_GRAM_TILE), (uint64_t *)result, (double2 *)(result + 16));
}

template <bool CPLX>
__global__ __launch_bounds__(256) void blend_kernel(char *ring, const uint64_t *__restrict__ offsets, const float *__restrict__ weights,
                                                    const BfBlendCell *__restrict__ cells, BfBlendArgs a)
{
	const uint32_t ci = row_of_block(cells, a.cells, &BfBlendCell::block_first, blockIdx.x);
	const BfBlendCell cell = cells[ci];
	const uint32_t tiles = a.padded_outputs / BF_MIX_TILE;
	const uint32_t block = blockIdx.x - cell.block_first, tile = block % tiles;
	const uint32_t v = (block / tiles) * 256u + threadIdx.x;
	if (v >= cell.volume) return;
	/* the voxel inside the cell, x fastest: its index along an axis is its r */
	const uint32_t rest = v / cell.count[0], x = v - rest * cell.count[0], z = rest / cell.count[1], y = rest - z * cell.count[1];
	const uint64_t e = ((uint64_t)(z + cell.first[2]) * a.points[1] + (y + cell.first[1])) * a.points[0] + (x + cell.first[0]);
	const float tx = (float)x * a.inv_step[0], ty = (float)y * a.inv_step[1], tz = (float)z * a.inv_step[2];

	const size_t node_floats = (size_t)tiles * a.frames * (2u * BF_MIX_TILE);
	float re[BF_MIX_TILE], im[BF_MIX_TILE];       /* the chains of the corner at hand */
	float xr[BF_MIX_TILE], xi[BF_MIX_TILE];       /* the stack: along x, */
	float yr[BF_MIX_TILE], yi[BF_MIX_TILE];       /* ... along y, */
	float zr[BF_MIX_TILE], zi[BF_MIX_TILE];       /* ... along z: the outputs */
	for (uint32_t cz = 0; cz < cell.corners[2]; cz++) {
		for (uint32_t cy = 0; cy < cell.corners[1]; cy++) {
			for (uint32_t cx = 0; cx < cell.corners[0]; cx++) {
				const uint32_t node = ((cell.node[2] + cz) * a.nodes[1] + (cell.node[1] + cy)) * a.nodes[0] + (cell.node[0] + cx);
				const float *w = weights + (size_t)node * node_floats + (size_t)tile * a.frames * (2u * BF_MIX_TILE);
				#pragma unroll
				for (uint32_t j = 0; j < BF_MIX_TILE; j++) { re[j] = 0.0f; im[j] = 0.0f; }
				for (uint32_t k = 0; k < a.frames; k++, w += 2u * BF_MIX_TILE) {
					const char *frame = ring + offsets[k];
					f32x2 c;
					if (CPLX) c = ((const f32x2 *)frame)[e];
					else      { c.x = ((const float *)frame)[e]; c.y = 0.0f; }
					mix_term<CPLX>(re, im, c, w);
				}
				#pragma unroll
				for (uint32_t j = 0; j < BF_MIX_TILE; j++) {
					if (cx == 0) { xr[j] = re[j]; if (CPLX) xi[j] = im[j]; }
					else         { xr[j] = __builtin_fmaf(tx, re[j] - xr[j], xr[j]); if (CPLX) xi[j] = __builtin_fmaf(tx, im[j] - xi[j], xi[j]); }
				}
			}
			#pragma unroll
			for (uint32_t j = 0; j < BF_MIX_TILE; j++) {
				if (cy == 0) { yr[j] = xr[j]; if (CPLX) yi[j] = xi[j]; }
				else         { yr[j] = __builtin_fmaf(ty, xr[j] - yr[j], yr[j]); if (CPLX) yi[j] = __builtin_fmaf(ty, xi[j] - yi[j], yi[j]); }
			}
		}
		#pragma unroll
		for (uint32_t j = 0; j < BF_MIX_TILE; j++) {
			if (cz == 0) { zr[j] = yr[j]; if (CPLX) zi[j] = yi[j]; }
			else         { zr[j] = __builtin_fmaf(tz, yr[j] - zr[j], zr[j]); if (CPLX) zi[j] = __builtin_fmaf(tz, yi[j] - zi[j], zi[j]); }
		}
	}
	char *out = ring + a.out_offset + (uint64_t)tile * BF_MIX_TILE * a.out_stride;
	const uint32_t rows = a.outputs - tile * BF_MIX_TILE;     /* (>= 1: the tiles cover padded_outputs) */
	#pragma unroll
	for (uint32_t j = 0; j < BF_MIX_TILE; j++, out += a.out_stride) {
		if (j < rows) {
			if (CPLX) { f32x2 c; c.x = zr[j]; c.y = zi[j]; ((f32x2 *)out)[e] = c; }
			else      ((float *)out)[e] = zr[j];
		}
	}
}

/* The other shape of the field mix, for lattices that do not blend along y (view planes: at most 4 corners a cell): each source voxel
 * is loaded ONCE a k and applied to every corner's chains -- four sets of 2 x 16 accumulators, slot 2 cz + cx, no stack --, and the lerps
 * close at the end, along x and then along z.  The chains and the lerps are blend_kernel's, operation for operation: the bytes are the
 * same.  A source voxel is read ceil(M / 16) times, not corners x ceil(M / 16) times; the price is a loop body of up to four corners'
 * weights, 128 scalar registers' worth of loads a k. */
template <bool CPLX>
__global__ __launch_bounds__(256) void blend_once_kernel(char *ring, const uint64_t *__restrict__ offsets, const float *__restrict__ weights,
                                                         const BfBlendCell *__restrict__ cells, BfBlendArgs a)
{
	const uint32_t ci = row_of_block(cells, a.cells, &BfBlendCell::block_first, blockIdx.x);
	const BfBlendCell cell = cells[ci];
	const uint32_t tiles = a.padded_outputs / BF_MIX_TILE;
	const uint32_t block = blockIdx.x - cell.block_first, tile = block % tiles;
	const uint32_t v = (block / tiles) * 256u + threadIdx.x;
	if (v >= cell.volume) return;
	const uint32_t rest = v / cell.count[0], x = v - rest * cell.count[0], z = rest / cell.count[1], y = rest - z * cell.count[1];
	const uint64_t e = ((uint64_t)(z + cell.first[2]) * a.points[1] + (y + cell.first[1])) * a.points[0] + (x + cell.first[0]);
	const float tx = (float)x * a.inv_step[0], tz = (float)z * a.inv_step[2];
	const bool two_x = cell.corners[0] == 2u, two_z = cell.corners[2] == 2u;

	const size_t node_floats = (size_t)tiles * a.frames * (2u * BF_MIX_TILE);
	const uint32_t node0 = (cell.node[2] * a.nodes[1] + cell.node[1]) * a.nodes[0] + cell.node[0];
	const float *w0 = weights + (size_t)node0 * node_floats + (size_t)tile * a.frames * (2u * BF_MIX_TILE);
	const float *w1 = w0 + (two_x ? node_floats : 0), *w2 = w0 + (two_z ? (size_t)a.nodes[0] * a.nodes[1] * node_floats : 0), *w3 = w2 + (two_x ? node_floats : 0);
	float r0[BF_MIX_TILE], i0[BF_MIX_TILE], r1[BF_MIX_TILE], i1[BF_MIX_TILE], r2[BF_MIX_TILE], i2[BF_MIX_TILE], r3[BF_MIX_TILE], i3[BF_MIX_TILE];
	#pragma unroll
	for (uint32_t j = 0; j < BF_MIX_TILE; j++) { r0[j] = i0[j] = r1[j] = i1[j] = r2[j] = i2[j] = r3[j] = i3[j] = 0.0f; }
	for (uint32_t k = 0; k < a.frames; k++) {
		const char *frame = ring + offsets[k];
		f32x2 c;
		if (CPLX) c = ((const f32x2 *)frame)[e];
		else      { c.x = ((const float *)frame)[e]; c.y = 0.0f; }
		const size_t at = (size_t)k * (2u * BF_MIX_TILE);
		mix_term<CPLX>(r0, i0, c, w0 + at);
		if (two_x) mix_term<CPLX>(r1, i1, c, w1 + at);
		if (two_z) {
			mix_term<CPLX>(r2, i2, c, w2 + at);
			if (two_x) mix_term<CPLX>(r3, i3, c, w3 + at);
		}
	}
	#pragma unroll
	for (uint32_t j = 0; j < BF_MIX_TILE; j++) {
		if (two_x) {
			r0[j] = __builtin_fmaf(tx, r1[j] - r0[j], r0[j]); if (CPLX) i0[j] = __builtin_fmaf(tx, i1[j] - i0[j], i0[j]);
			if (two_z) { r2[j] = __builtin_fmaf(tx, r3[j] - r2[j], r2[j]); if (CPLX) i2[j] = __builtin_fmaf(tx, i3[j] - i2[j], i2[j]); }
		}
		if (two_z) { r0[j] = __builtin_fmaf(tz, r2[j] - r0[j], r0[j]); if (CPLX) i0[j] = __builtin_fmaf(tz, i2[j] - i0[j], i0[j]); }
	}
	char *out = ring + a.out_offset + (uint64_t)tile * BF_MIX_TILE * a.out_stride;
	const uint32_t rows = a.outputs - tile * BF_MIX_TILE;
	#pragma unroll
	for (uint32_t j = 0; j < BF_MIX_TILE; j++, out += a.out_stride) {
		if (j < rows) {
			if (CPLX) { f32x2 c; c.x = r0[j]; c.y = i0[j]; ((f32x2 *)out)[e] = c; }
			else      ((float *)out)[e] = r0[j];
		}
	}
}

/* Every table but host_boxes is device memory.  Every box lies inside every frame and every frame inside the ring: the caller's business
 * (frame_ops.cpp: gram_boxes_last_frames); what is checked here is what bf_launch_gram checks of its arguments, box by box, and that the
 * prefixes are the sums of the boxes' block counts -- a block that found no box of its own would index past a table. */
extern "C" hipError_t bf_launch_gram_boxes(const void *ring, const uint64_t *offsets, const BfBlocksBox *host_boxes, const BfBlocksBox *boxes,
                                           uint32_t box_count, uint32_t mask_blocks, uint32_t partial_blocks, uint64_t *mask, double *partials,
                                           void *results, hipStream_t s)
{
	if (!ring || !offsets || !host_boxes || !boxes || !mask || !partials || !results || box_count == 0 || box_count > BF_BLOCKS_MAX_BOXES)
		return hipErrorInvalidValue;
	const uint32_t frames = host_boxes[0].a.frames;
	uint64_t mask_sum = 0, partial_sum = 0;
	for (uint32_t b = 0; b < box_count; b++) {
		const BfBlocksBox &row = host_boxes[b];
		const BfGramArgs *a = &row.a;
		if (a->frames != frames || a->frames == 0 || a->frames > BF_ENSEMBLE_MAX_FRAMES || a->volume == 0 ||
		    a->words != (uint32_t)(((uint64_t)a->volume + BF_GRAM_WORD - 1u) / BF_GRAM_WORD) || a->chunk_words == 0 ||
		    a->chunks != (a->words + a->chunk_words - 1u) / a->chunk_words || a->tiles != bf_gram_tiles(a->frames) ||
		    a->tile_pairs != bf_gram_tile_pairs(a->frames) || row.mask_block_first != mask_sum || row.partial_block_first != partial_sum)
			return hipErrorInvalidValue;
		mask_sum += (a->words + 3u) / 4u;
		partial_sum += (uint64_t)a->chunks * a->tile_pairs;
		if (mask_sum > 0x7FFFFFFFull || partial_sum > 0x7FFFFFFFull) return hipErrorInvalidValue;
	}
	if (mask_sum != mask_blocks || partial_sum != partial_blocks) return hipErrorInvalidValue;
	hipLaunchKernelGGL(blocks_mask_kernel, dim3(mask_blocks), dim3(256), 0, s, (const char *)ring, offsets, boxes, box_count, mask);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(blocks_partial_kernel, dim3(partial_blocks), dim3(256), 0, s, (const char *)ring, offsets, boxes, box_count,
	                   (const uint64_t *)mask, (double2 *)partials);
	e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(blocks_fold_kernel, dim3((frames + 63u) / 64u, frames + 1u, box_count), dim3(64), 0, s, boxes, (const uint64_t *)mask,
	                   (const double2 *)partials, (char *)results);
	return hipGetLastError();
}

/* Every table is device memory.  The cells tile the frame, their prefix ends in a->blocks, every node they name lies inside the lattice,
 * every frame and the output run inside the ring, the output run clear of the source frames: the caller's business (frame_ops.cpp:
 * mix_field_last_frames), nothing here re-checks it. */
extern "C" hipError_t bf_launch_blend(void *ring, const uint64_t *offsets, const float *weights, const BfBlendCell *cells, const BfBlendArgs *a,
                                      hipStream_t s)
{
	if (!ring || !offsets || !weights || !cells || !a || a->frames == 0 || a->frames > BF_ENSEMBLE_MAX_FRAMES || a->outputs == 0 ||
	    a->outputs > BF_ENSEMBLE_MAX_FRAMES || a->padded_outputs != (a->outputs + BF_MIX_TILE - 1u) / BF_MIX_TILE * BF_MIX_TILE ||
	    a->cells == 0 || a->blocks == 0 || a->blocks > 0x7FFFFFFFu || !a->nodes[0] || !a->nodes[1] || !a->nodes[2] ||
	    (uint64_t)a->nodes[0] * a->nodes[1] * a->nodes[2] > BF_BLEND_MAX_NODES)
		return hipErrorInvalidValue;
	if (a->once && a->nodes[1] != 1u) return hipErrorInvalidValue;       /* blend_once_kernel has no lerp along y */
	if (a->once) {
		if (a->cplx) hipLaunchKernelGGL(blend_once_kernel<true>, dim3(a->blocks), dim3(256), 0, s, (char *)ring, offsets, weights, cells, *a);
		else         hipLaunchKernelGGL(blend_once_kernel<false>, dim3(a->blocks), dim3(256), 0, s, (char *)ring, offsets, weights, cells, *a);
		return hipGetLastError();
	}
	if (a->cplx) hipLaunchKernelGGL(blend_kernel<true>, dim3(a->blocks), dim3(256), 0, s, (char *)ring, offsets, weights, cells, *a);
	else         hipLaunchKernelGGL(blend_kernel<false>, dim3(a->blocks), dim3(256), 0, s, (char *)ring, offsets, weights, cells, *a);
	return hipGetLastError();
}
