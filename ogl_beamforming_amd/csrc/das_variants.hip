/* das_variants.hip -- the general kernel (das.hip) for several DAS SCALAR SETS: one DAS input beamformed on the block's own grid under K
 * triples of speed of sound, time offset and f-number by one launch (beamformer_hip_push_data_variants_with_compute; sound-speed
 * autofocus, system-delay calibration, f-number tuning: the same RF under K candidate values, the sharpest or most coherent kept).
 *
 * Grid x: the 256-voxel tiles of the block's grid, in general_tile_at's walk order (das_general.h) -- no dealing to the XCDs, no channel
 * split: a split or a dealing chosen from the total would make a variant's bits depend on its company.  Grid y: the taken variant.  A
 * block reads what differs from variant to variant from its BfVariantRow (32 bytes, the same for every lane: scalar loads, the fields
 * live in SGPRs for the whole loop), copies the launch's BfDasArgs, overrides those five fields and the frame, and then IS a block of the
 * general kernel: the prologue (tile_voxel, voxel_point), das_rca over all channels -- settle_index reads the overridden arguments, so the row
 * ends follow each variant's own speed and margin -- and the epilogue's value (coherency_weighted) are the functions das.hip calls.  No
 * LDS, no barrier.
 *
 * A variant's bits depend on the DAS input, the parameter block and its own triple: not on how many variants the launch holds, nor on
 * their order.  RCA family only (RCA_TPW, RCA_VLS, Flash): 3 interpolation modes x real / IQ x with / without coherency weighting = 12
 * instantiations.
 */
#include "das_general.h"

template <int INTERP, bool CPLX, bool CW>
__global__ __launch_bounds__(256) void das_variants_kernel(const BfDasArgs base, const BfVariantRow *const __restrict__ rows)
{
	const BfVariantRow &row = rows[blockIdx.y];

	BfDasArgs p = base;
	p.speed_of_sound = row.speed_of_sound; p.inv_speed_of_sound = row.inv_speed_of_sound;
	p.time_offset = row.time_offset; p.f_number = row.f_number; p.edge_margin = row.edge_margin;
	p.out = (char *)base.out + row.out_offset;

	const GeneralTile tile = general_tile_at(p, blockIdx.x);
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

/* `a`: the block's general-kernel arguments with 256-voxel tiles and no channel split, rf the DAS input, out the first taken variant's
 * frame; rows: variant_count rows on the device (bf_launch_views_table put them there) */
extern "C" hipError_t bf_launch_das_variants(const BfDasArgs *a, const BfVariantRow *rows, uint32_t variant_count, hipStream_t s)
{
	const uint64_t tiles = (uint64_t)a->blocks[0] * a->blocks[1] * a->blocks[2];
	if (a->family != BF_DAS_RCA || a->split_shift || a->depth_major > 2u || a->z_first != 0 || a->z_count != a->size[2] || !rows ||
	    variant_count == 0 || variant_count > 65535u || tiles == 0 || tiles > 0x7FFFFFFFu) return hipErrorInvalidValue;
	return bf_dispatch_kind(a, [&](auto interp, auto cplx, auto cw) {
		hipLaunchKernelGGL((das_variants_kernel<interp, cplx, cw>), dim3((uint32_t)tiles, variant_count), dim3(256), 0, s, *a, rows);
		return hipGetLastError();
	});
}
