/* das_burst_views.hip -- the burst kernel (das_burst.hip) for an ensemble on several GRIDS: N RF frames of one geometry beamformed on K
 * voxel grids by one launch (beamformer_hip_push_data_burst_views_with_compute).  12 instantiations, as das_burst_kernel's.  A file of
 * its own: compiled beside the kernels of das_burst.hip it changed one of them by an instruction, and those stay what they were. */
#include "das_burst_term.h"

/* das_burst_kernel on the tiles of several GRIDS (beamformer_hip_push_data_burst_views_with_compute: an ensemble on K grids -- bi-plane
 * and tri-plane ultrafast imaging, an ULM ensemble refined on one set of patches).  Grid x: the 256-voxel tiles of all taken views,
 * concatenated exactly as das_views.hip does -- view v owns the block ids first_block[v] .. first_block[v + 1] - 1 in its own walk order,
 * found by a binary search over scalar loads, its BfViewRow's fields held in SGPRs, no dealing to the XCDs; grid y: groups of FB frames.
 * Thread to voxel, voxel to point, the frames of the block, the term and the epilogue's value are the shared helpers (das_general.h,
 * das_common.h, das_burst_term.h).  Two pieces stay restated, text for text: the view of the block (das_views.hip's; shared as a function
 * that returns the view, the index alone or the overridden arguments, it gave every kernel of both files other registers with this
 * compiler) and the RCA loop (das_burst_kernel's; shared as das_rca_burst(p, rf, wx, wy, wz, x, y, z, acc) it changed every kernel of
 * both files).  Frame f of a view reads rf + f * rf_stride and writes the view's frame + f * the
 * ROW's out_stride: a view's frames lie one behind the other in the frame ring, the views' runs follow one another.  A frame's bits
 * depend on its RF, the parameter block and its view's grid: not on its slot, nor on the other views or their order. */
template <int INTERP, bool CPLX, bool CW>
__global__ __launch_bounds__(256) void das_burst_views_kernel(const BfDasArgs base, const BfViewRow *const __restrict__ rows,
                                                              const uint32_t *const __restrict__ first_block, const uint32_t view_count,
                                                              const uint32_t frame_count, const uint64_t rf_stride)
{
	/* the view of this block: the last v with first_block[v] <= blockIdx.x (das_views.hip) */
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
	const uint64_t out_stride = row.out_stride;

	const GeneralTile tile = general_tile_at(p, bid - first_block[lo]);
	uint32_t x, y, z;
	tile_voxel(p, tile, threadIdx.x, x, y, z);
	if (!(x < p.size[0] && y < p.size[1] && z < p.size[2])) return;

	/* this block's frames: first .. first + count - 1; the spare slots of a short last group alias its last frame */
	uint32_t first, count;
	burst_frames(frame_count, first, count);
	const char *rf[FB];
	for (int f = 0; f < FB; f++) {
		const uint32_t frame = first + ((uint32_t)f < count ? (uint32_t)f : count - 1u);
		rf[f] = (const char *)p.rf + (uint64_t)frame * rf_stride;
	}
	Accumulator<CPLX, CW, false> acc[FB];
	for (int f = 0; f < FB; f++) acc[f].init();

	float wx, wy, wz;
	voxel_point(p, x, y, z, wx, wy, wz);

	/* das.glsl:204-231 */
	float xx, xy, xz;
	m4_point(p.xdc_transform, wx, wy, wz, xx, xy, xz);
	const int S = p.sample_count, A = p.acquisition_count, C = p.channel_count;
	const float inv_abs_z = hw_rcp(__builtin_fabsf(xz));
	const float zz = xz * xz;

	for (int acquisition = 0; acquisition < A; acquisition++) {
		const BfTransmit t = p.transmits[acquisition];
		const bool  rx_rows = (t.flags & BF_RX_ROWS) != 0;
		const float lateral = rx_rows ? xy : xx;
		const float pitch   = rx_rows ? p.pitch[1] : p.pitch[0];
		const float tx_dist = transmit_distance(t, wx, wy, wz);
		const float f_over_z = p.f_number * inv_abs_z;

		int rf_offset = acquisition * S;
		for (int channel = 0; channel < C; channel++) {
			float dx    = lateral - (float)channel * pitch;
			float a_arg = __builtin_fabsf(dx * f_over_z);
			if (a_arg < 0.5f) {
				float sidx = sample_index(tx_dist + hw_sqrt(dx * dx + zz), p);
				sidx = settle_index<BF_DAS_RCA, INTERP>(sidx, p, x, y, z, channel, acquisition);
				burst_term<INTERP, CPLX, CW>(rf, rf_offset, sidx, apodize(a_arg), p, acc);
			}
			rf_offset += S * A;
		}
	}

	const uint64_t out_index = (uint64_t)p.size[0] * p.size[1] * z + (uint64_t)p.size[0] * y + x;
	for (int f = 0; f < FB; f++) {
		if ((uint32_t)f < count) {
			reinterpret_cast<sample_t<CPLX> *>((char *)p.out + (uint64_t)(first + (uint32_t)f) * out_stride)[out_index] = coherency_weighted<CW>(acc[f].coherent, acc[f].incoherent);
		}
	}
}

/* `a` as for bf_launch_das_views (rf: the first RF frame's DAS input, out: the first taken view's first frame); b: the frame count and
 * the input's stride; `v`: the rows (each with its out_stride) and the prefix table, total_blocks = first_block[view_count] */
extern "C" hipError_t bf_launch_das_burst_views(const BfDasArgs *a, const BfBurstArgs *b, const BfViewsArgs *v, uint32_t total_blocks, hipStream_t s)
{
	const uint32_t groups = (b->frame_count + BF_BURST_FRAMES_PER_THREAD - 1u) / BF_BURST_FRAMES_PER_THREAD;
	if (a->family != BF_DAS_RCA || a->split_shift || b->frame_count == 0 || groups > 65535u || v->view_count == 0 || total_blocks == 0 ||
	    total_blocks > 0x7FFFFFFFu || !v->rows || !v->first_block) return hipErrorInvalidValue;
	return bf_dispatch_kind(a, [&](auto interp, auto cplx, auto cw) {
		hipLaunchKernelGGL((das_burst_views_kernel<interp, cplx, cw>), dim3(total_blocks, groups), dim3(256), 0, s, *a, v->rows, v->first_block, v->view_count,
		                   b->frame_count, b->rf_stride);
		return hipGetLastError();
	});
}
