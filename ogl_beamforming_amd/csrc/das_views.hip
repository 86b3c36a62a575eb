/* das_views.hip -- the general kernel (das.hip) for several GRIDS: one DAS input beamformed on K voxel grids by one launch
 * (beamformer_hip_push_data_views_with_compute; live X-plane / tri-plane imaging, and the ULM use: tens to hundreds of small fine
 * patches around detections, all from the RF of one push).
 *
 * A patch of 16 x 16 voxels is ONE block of the general kernel, and a launch of that class costs about 14 us whatever it computes
 * (DESIGN 3.1a).  Here the tiles of all views are concatenated along grid x: view v owns the block ids first_block[v] ..
 * first_block[v + 1] - 1, in that view's own walk order (general_tile_at, das_general.h).  No dealing to the XCDs and so no padded ids:
 * a patch is 1-4 blocks.  A block finds its view by a binary search over first_block[] -- K + 1 words in global memory, the same for
 * every lane, so the loads are scalar loads -- and reads what differs from view to view from that view's BfViewRow (128 bytes, scalar
 * loads again: the fields live in SGPRs for the whole loop).  It then IS a block of the general kernel on that grid: the prologue
 * (tile_voxel, das_general.h; voxel_point, das_common.h), das_rca over all channels (das_general.h: the general kernel's own loop,
 * row-end settlement included) and the epilogue's value (coherency_weighted, das_common.h) are the functions das.hip calls.  (The view
 * search and the override below are restated in das_burst_views.hip: see there.)  No channel split -- the views fill the chip as frames do in das_burst.hip, and
 * a split chosen from the total would make a view's bits depend on its company --, no LDS, no barrier.
 *
 * A view's bits depend on the DAS input, the parameter block and its own grid: not on how many views the launch holds, nor on their
 * order.  RCA family only (RCA_TPW, RCA_VLS, Flash): 3 interpolation modes x real / IQ x with / without coherency weighting = 12
 * instantiations.
 */
#include "das_general.h"

template <int INTERP, bool CPLX, bool CW>
__global__ __launch_bounds__(256) void das_views_kernel(const BfDasArgs base, const BfViewRow *const __restrict__ rows,
                                                        const uint32_t *const __restrict__ first_block, const uint32_t view_count)
{
	/* the view of this block: the last v with first_block[v] <= blockIdx.x (views without tiles do not occur: every extent >= 1) */
	const uint32_t bid = blockIdx.x;
	uint32_t lo = 0, hi = view_count;
	while (hi - lo > 1u) {
		const uint32_t mid = (lo + hi) >> 1;
		if (first_block[mid] <= bid) lo = mid; else hi = mid;
	}
	const BfViewRow &row = rows[lo];

	BfDasArgs p = base;
	for (int k = 0; k < 16; k++) p.voxel_transform[k] = row.voxel_transform[k];
	for (int k = 0; k < 3; k++) { p.size[k] = row.size[k]; p.tile_shift[k] = row.tile_shift[k]; p.blocks[k] = row.blocks[k]; }
	p.depth_major = row.depth_major; p.band_rows = row.band_rows;
	p.z_first = 0; p.z_count = row.size[2];
	p.out = (char *)base.out + row.out_offset;

	const GeneralTile tile = general_tile_at(p, bid - first_block[lo]);
	uint32_t x, y, z;
	tile_voxel(p, tile, threadIdx.x, x, y, z);
	/* (the shifts of a tile sum to 8: a grid of fewer than 256 voxels gives the spare ones to x, and those lanes fall outside) */
	if (!(x < p.size[0] && y < p.size[1] && z < p.size[2])) return;

	Accumulator<CPLX, CW, false> acc;
	acc.init();
	float wx, wy, wz;
	voxel_point(p, x, y, z, wx, wy, wz);
	das_rca<INTERP, CPLX, CW, false>(p, (const char *)p.rf, wx, wy, wz, x, y, z, 0, p.channel_count, acc);

	uint64_t out_index = (uint64_t)p.size[0] * p.size[1] * z + (uint64_t)p.size[0] * y + x;
	reinterpret_cast<sample_t<CPLX> *>(p.out)[out_index] = coherency_weighted<CW>(acc.coherent, acc.incoherent);
}

/* The rows and the prefix table of a push, from the pinned memory the host wrote them to (`src`: its device-side address) into the
 * device table: a few KB read in place over PCIe by one small launch, in order on the push's stream.  (A copy-engine transfer and its
 * cross-queue dependency cost 40-60 us here -- executor.cpp, kOverlapBytes -- more than the whole DAS stage of a push of patches.) */
__global__ __launch_bounds__(256) void views_table_kernel(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, uint32_t words)
{
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < words; i += gridDim.x * 256u) dst[i] = src[i];
}

extern "C" hipError_t bf_launch_views_table(void *dst, const void *src, uint32_t bytes, hipStream_t s)
{
	const uint32_t words = (bytes + 3u) / 4u, blocks = (words + 255u) / 256u;
	if (!dst || !src || !words) return hipErrorInvalidValue;
	hipLaunchKernelGGL(views_table_kernel, dim3(blocks < 64u ? blocks : 64u), dim3(256), 0, s, (uint32_t *)dst, (const uint32_t *)src, words);
	return hipGetLastError();
}

/* `a`: the block's general-kernel arguments (everything but the grid), rf the DAS input, out the first view's frame; `v`: the rows and
 * the prefix table, total_blocks = first_block[view_count] */
extern "C" hipError_t bf_launch_das_views(const BfDasArgs *a, const BfViewsArgs *v, uint32_t total_blocks, hipStream_t s)
{
	if (a->family != BF_DAS_RCA || v->view_count == 0 || total_blocks == 0 || !v->rows || !v->first_block) return hipErrorInvalidValue;
	return bf_dispatch_kind(a, [&](auto interp, auto cplx, auto cw) {
		hipLaunchKernelGGL((das_views_kernel<interp, cplx, cw>), dim3(total_blocks), dim3(256), 0, s, *a, v->rows, v->first_block, v->view_count);
		return hipGetLastError();
	});
}
