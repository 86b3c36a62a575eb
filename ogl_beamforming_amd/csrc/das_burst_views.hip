/* das_burst_views.hip -- the burst kernel (das_burst.hip) for an ensemble on several GRIDS: N RF frames of one geometry beamformed on K
 * voxel grids by one launch (beamformer_hip_push_data_burst_views_with_compute).  12 instantiations, as das_burst_kernel's.  A file of
 * its own: compiled beside the kernels of das_burst.hip it changed one of them by an instruction, and those stay what they were. */
#include "das_burst_term.h"

/* das_burst_kernel on the tiles of several GRIDS (beamformer_hip_push_data_burst_views_with_compute: an ensemble on K grids -- bi-plane
 * and tri-plane ultrafast imaging, an ULM ensemble refined on one set of patches).  Grid x: the 256-voxel tiles of all taken views,
 * concatenated exactly as das_views.hip does -- view v owns the block ids first_block[v] .. first_block[v + 1] - 1 in its own walk order,
 * found by a binary search over scalar loads, its BfViewRow's fields held in SGPRs, no dealing to the XCDs; grid y: groups of FB frames.
 * The body below the tile is das_burst_kernel's, text for text: restated, not shared through a function, so that the old kernel's code
 * stays what it was (general_tile beside general_tile_at, das_general.h, is the precedent).  Frame f of a view reads rf + f * rf_stride and writes the view's frame + f * the
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
	const uint32_t bx = tile.bx, by = tile.by, bz = tile.bz;

	uint32_t tid = threadIdx.x;
	uint32_t lx  = tid & ((1u << p.tile_shift[0]) - 1u);
	uint32_t ly  = (tid >> p.tile_shift[0]) & ((1u << p.tile_shift[1]) - 1u);
	uint32_t lz  = (tid >> (p.tile_shift[0] + p.tile_shift[1])) & ((1u << p.tile_shift[2]) - 1u);
	uint32_t x = (bx << p.tile_shift[0]) + lx;
	uint32_t y = (by << p.tile_shift[1]) + ly;
	uint32_t z = (bz << p.tile_shift[2]) + lz;
	if (!(x < p.size[0] && y < p.size[1] && z < p.size[2])) return;

	/* this block's frames: first .. first + count - 1; the spare slots of a short last group alias its last frame */
	const uint32_t first = blockIdx.y * (uint32_t)FB;
	const uint32_t count = frame_count - first < (uint32_t)FB ? frame_count - first : (uint32_t)FB;
	const char *rf[FB];
	for (int f = 0; f < FB; f++) {
		const uint32_t frame = first + ((uint32_t)f < count ? (uint32_t)f : count - 1u);
		rf[f] = (const char *)p.rf + (uint64_t)frame * rf_stride;
	}
	Accumulator<CPLX, CW, false> acc[FB];
	for (int f = 0; f < FB; f++) acc[f].init();

	/* das.glsl:374-376 */
	float px = (float)x / fmaxf(1.0f, (float)p.size[0] - 1.0f);
	float py = (float)y / fmaxf(1.0f, (float)p.size[1] - 1.0f);
	float pz = (float)z / fmaxf(1.0f, (float)p.size[2] - 1.0f);
	float wx, wy, wz;
	m4_point(p.voxel_transform, px, py, pz, wx, wy, wz);

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
			sample_t<CPLX> v = acc[f].coherent;
			/* coherency_weighting.glsl:36 with Scale = 1 (beamformer_core.c:949), as das.hip's epilogue */
			if constexpr (CW) v = v * (v / acc[f].incoherent);
			reinterpret_cast<sample_t<CPLX> *>((char *)p.out + (uint64_t)(first + (uint32_t)f) * out_stride)[out_index] = v;
		}
	}
}

template <int INTERP, bool CPLX, bool CW>
static hipError_t launch_views_one(const BfDasArgs *a, const BfBurstArgs *b, const BfViewsArgs *v, uint32_t total_blocks, hipStream_t s)
{
	uint32_t groups = (b->frame_count + BF_BURST_FRAMES_PER_THREAD - 1u) / BF_BURST_FRAMES_PER_THREAD;
	hipLaunchKernelGGL((das_burst_views_kernel<INTERP, CPLX, CW>), dim3(total_blocks, groups), dim3(256), 0, s, *a, v->rows, v->first_block, v->view_count,
	                   b->frame_count, b->rf_stride);
	return hipGetLastError();
}

template <int INTERP>
static hipError_t launch_views_kind(const BfDasArgs *a, const BfBurstArgs *b, const BfViewsArgs *v, uint32_t total_blocks, hipStream_t s)
{
	if (a->complex_data) return a->coherency_weighting ? launch_views_one<INTERP, true,  true>(a, b, v, total_blocks, s) : launch_views_one<INTERP, true,  false>(a, b, v, total_blocks, s);
	else                 return a->coherency_weighting ? launch_views_one<INTERP, false, true>(a, b, v, total_blocks, s) : launch_views_one<INTERP, false, false>(a, b, v, total_blocks, s);
}

/* `a` as for bf_launch_das_views (rf: the first RF frame's DAS input, out: the first taken view's first frame); b: the frame count and
 * the input's stride; `v`: the rows (each with its out_stride) and the prefix table, total_blocks = first_block[view_count] */
extern "C" hipError_t bf_launch_das_burst_views(const BfDasArgs *a, const BfBurstArgs *b, const BfViewsArgs *v, uint32_t total_blocks, hipStream_t s)
{
	const uint32_t groups = (b->frame_count + BF_BURST_FRAMES_PER_THREAD - 1u) / BF_BURST_FRAMES_PER_THREAD;
	if (a->family != BF_DAS_RCA || a->split_shift || b->frame_count == 0 || groups > 65535u || v->view_count == 0 || total_blocks == 0 ||
	    total_blocks > 0x7FFFFFFFu || !v->rows || !v->first_block) return hipErrorInvalidValue;
	switch (a->interpolation) {
	case BF_INTERP_NEAREST: return launch_views_kind<BF_INTERP_NEAREST>(a, b, v, total_blocks, s);
	case BF_INTERP_LINEAR:  return launch_views_kind<BF_INTERP_LINEAR>(a, b, v, total_blocks, s);
	case BF_INTERP_CUBIC:   return launch_views_kind<BF_INTERP_CUBIC>(a, b, v, total_blocks, s);
	}
	return hipErrorInvalidValue;
}
