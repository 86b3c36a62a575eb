/* das_general.h -- what the general kernel (das.hip) and its forms for an ensemble (das_burst.hip), for several grids (das_views.hip),
 * for an ensemble on several grids (das_burst_views.hip) and for several scalar sets (das_variants.hip) share.  One text, so that a frame
 * of a burst, a view and a variant are the same arithmetic as a single frame:
 *   Accumulator, transmit_distance, sample_index, settle_index   all five (transmit_distance: das_factored.hip too)
 *   das_rca (the RCA family's loop)                               das.hip, das_views.hip, das_variants.hip
 *   general_tile (block id -> tile, dealt to the XCDs)            das.hip, das_burst.hip (both kernels)
 *   general_tile_at (tile number -> tile)                         das_views.hip, das_burst_views.hip, das_variants.hip
 *   tile_voxel (thread -> voxel)                                  das_views.hip, das_burst_views.hip, das_variants.hip, das_tile.hip;
 *                                                                 das.hip, das_burst.hip and das_factored.hip restate it (the call
 *                                                                 compiled to other code there: see those files)
 * The voxel's point (voxel_point), the epilogue's value (coherency_weighted) and the launchers' template dispatch (bf_dispatch_kind) are
 * das_common.h's, the grid size (bf_general_grid_blocks) is bf_kernels.h's: the fast kernels use them too. */
#ifndef BF_DAS_GENERAL_H
#define BF_DAS_GENERAL_H

#include "das_exact.h"

template <bool CPLX, bool CW, bool COUNT>
struct Accumulator {
	sample_t<CPLX> coherent;
	float          incoherent;
	unsigned long long pairs;
	__device__ __forceinline__ void init() { coherent = zero_sample<CPLX>(); incoherent = 0.f; pairs = 0; }
	/* RESULT_STORE (das.glsl:28-32) */
	__device__ __forceinline__ void add(sample_t<CPLX> v)
	{
		coherent += v;
		if constexpr (CW) {
			if constexpr (CPLX) incoherent += hw_sqrt(v.x * v.x + v.y * v.y);
			else                incoherent += __builtin_fabsf(v);
		}
	}
};

/* das.glsl:187-202 with the per-transmit constants precomputed */
__device__ __forceinline__ float transmit_distance(const BfTransmit &t, float wx, float wy, float wz)
{
	float result = 0.f;
	if (!(t.flags & BF_TX_NONE)) {
		float px = (t.flags & BF_TX_ROWS) ? wy : wx;
		if (t.flags & BF_TX_PLANE) {
			result = px * t.sin_a + wz * t.cos_a;
		} else {
			float dx = px - t.focus_x, dz = wz - t.focus_z;
			result = hw_sqrt(dx * dx + dz * dz);
		}
	}
	return result;
}

/* das.glsl:126-130 */
__device__ __forceinline__ float sample_index(float distance, const BfDasArgs &p)
{
	return (div_speed_of_sound(distance, p) + p.time_offset) * p.sampling_frequency;
}

/* A term at an end of its RF row (das_exact.h): this kernel's index -- hardware square root, fused multiply-adds -- may differ
 * from the shader's by an ulp, and sample_rf's range test is a step.  Within p.edge_margin of either end the index is therefore
 * formed again, exactly as the shader's text forms it; everything else about the term stays as it is.  (Nearest interpolation:
 * the index decides the tap at every half-integer, not only at the row ends -- the parity tests budget those flips per voxel.) */
template <int FAMILY, int INTERP>
__device__ __forceinline__ float settle_index(float index, const BfDasArgs &p, uint32_t x, uint32_t y, uint32_t z, int channel, int transmit)
{
	if constexpr (INTERP != BF_INTERP_NEAREST) {
		if (bfx::edge_near<INTERP>(index, p.sample_count, p.edge_margin))
			index = bfx::exact_index<FAMILY>(p, bfx::exact_voxel<FAMILY>(p, x, y, z), channel, transmit);
	}
	return index;
}

/* das.glsl:204-231 */
template <int INTERP, bool CPLX, bool CW, bool COUNT>
__device__ __forceinline__ void das_rca(const BfDasArgs &p, const char *rf, float wx, float wy, float wz, uint32_t x, uint32_t y, uint32_t z,
                                        int ch0, int ch1, Accumulator<CPLX, CW, COUNT> &acc)
{
	float xx, xy, xz;
	m4_point(p.xdc_transform, wx, wy, wz, xx, xy, xz);
	const int S = p.sample_count, A = p.acquisition_count;
	const float inv_abs_z = hw_rcp(__builtin_fabsf(xz));
	const float zz = xz * xz;

	for (int acquisition = 0; acquisition < A; acquisition++) {
		const BfTransmit t = p.transmits[acquisition];
		const bool  rx_rows = (t.flags & BF_RX_ROWS) != 0;
		const float lateral = rx_rows ? xy : xx;
		const float pitch   = rx_rows ? p.pitch[1] : p.pitch[0];
		const float tx_dist = transmit_distance(t, wx, wy, wz);
		const float f_over_z = p.f_number * inv_abs_z;

		int rf_offset = acquisition * S + ch0 * S * A;
		for (int channel = ch0; channel < ch1; channel++) {
			float dx    = lateral - (float)channel * pitch;
			float a_arg = __builtin_fabsf(dx * f_over_z);
			bool  pass  = a_arg < 0.5f;
			if constexpr (COUNT) {
				acc.pairs += pass;
			} else if (pass) {
				float sidx = sample_index(tx_dist + hw_sqrt(dx * dx + zz), p);
				sidx = settle_index<BF_DAS_RCA, INTERP>(sidx, p, x, y, z, channel, acquisition);
				acc.add(apodize(a_arg) * sample_rf<INTERP, CPLX>(rf, rf_offset, sidx, p));
			}
			rf_offset += S * A;
		}
	}
}

/* Block id -> tile (bx, by, bz) of the general kernel's grid; valid false: a block of the ragged tail, which has no tile.
 * (One of six copies of this walk; tests/walk_cases.py pins each at the tile counts and band counts where its branches differ.) */
struct GeneralTile { uint32_t bx, by, bz; bool valid; };
__device__ __forceinline__ GeneralTile general_tile(const BfDasArgs &p, uint32_t bid)
{
	uint32_t bx = 0, by = 0, bz = 0;
	/* blockIdx -> tile: consecutive block ids go round-robin over the 8 XCDs, so ids that
	 * share (id % 8) share an L2.  Deal the tile list out so that each XCD walks a
	 * contiguous run of tiles (neighbouring tiles read neighbouring RF windows). */
	uint32_t total  = p.blocks[0] * p.blocks[1] * p.blocks[2];
	uint32_t per    = (total + 7u) / 8u;
	uint32_t tile   = (bid & 7u) * per + (bid >> 3);
	if (p.depth_major != 3u && tile >= total) {
		/* ragged tail: ids whose run is shorter map onto the unassigned remainder */
		return GeneralTile{0, 0, 0, false};
	}
	/* depth-major walk: consecutive tiles (in flight together on an XCD) are one lateral column at
	 * consecutive depths, whose RF windows overlap almost entirely (das_separable.hip) */
	if (p.depth_major == 3u) {
		bz = 0;
		if (!bf_plane_walk(bid, p.blocks[0], p.blocks[1], p.band_rows, bx, by)) return GeneralTile{0, 0, 0, false};     /* whole block */
	} else if (p.depth_major == 2u) {
		/* view planes (depth on voxel y, one voxel along z): y fastest, so that each XCD's run of tiles is a lateral COLUMN
		 * at every depth -- the work per tile grows with depth (f-number culling), a run of depth ROWS would leave the XCDs
		 * that hold the shallow rows idle for a fifth of the launch */
		by = tile % p.blocks[1];
		bx = (tile / p.blocks[1]) % p.blocks[0];
		bz = tile / (p.blocks[1] * p.blocks[0]);
	} else if (p.depth_major) {
		bz = tile % p.blocks[2];
		bx = (tile / p.blocks[2]) % p.blocks[0];
		by = tile / (p.blocks[2] * p.blocks[0]);
	} else {
		bx = tile % p.blocks[0];
		by = (tile / p.blocks[0]) % p.blocks[1];
		bz = tile / (p.blocks[0] * p.blocks[1]);
	}
	return GeneralTile{bx, by, bz, true};
}

/* Tile NUMBER (below blocks[0] * blocks[1] * blocks[2]) -> tile, in the walk order depth_major 0, 1 or 2 names: general_tile's second
 * half without its dealing of block ids to the XCDs.  das_views.hip, whose blocks take the tiles of several grids in turn, enters here.
 * (general_tile keeps its own text: split in two it compiled to other code, and a single frame's kernels stay as they are.) */
__device__ __forceinline__ GeneralTile general_tile_at(const BfDasArgs &p, uint32_t tile)
{
	uint32_t bx = 0, by = 0, bz = 0;
	if (p.depth_major == 2u) {
		by = tile % p.blocks[1];
		bx = (tile / p.blocks[1]) % p.blocks[0];
		bz = tile / (p.blocks[1] * p.blocks[0]);
	} else if (p.depth_major) {
		bz = tile % p.blocks[2];
		bx = (tile / p.blocks[2]) % p.blocks[0];
		by = tile / (p.blocks[2] * p.blocks[0]);
	} else {
		bx = tile % p.blocks[0];
		by = (tile / p.blocks[0]) % p.blocks[1];
		bz = tile / (p.blocks[0] * p.blocks[1]);
	}
	return GeneralTile{bx, by, bz, true};
}

/* Thread `tid` of the block on `tile` -> its voxel (x, y, z): z counts inside the shard.  The range test stays with the caller.
 * (Out-parameters, the tile copied to locals first: returned as a struct the same text compiled to other code.) */
__device__ __forceinline__ void tile_voxel(const BfDasArgs &p, const GeneralTile &tile, uint32_t tid, uint32_t &x, uint32_t &y, uint32_t &z)
{
	const uint32_t bx = tile.bx, by = tile.by, bz = tile.bz;
	uint32_t lx  = tid & ((1u << p.tile_shift[0]) - 1u);
	uint32_t ly  = (tid >> p.tile_shift[0]) & ((1u << p.tile_shift[1]) - 1u);
	uint32_t lz  = (tid >> (p.tile_shift[0] + p.tile_shift[1])) & ((1u << p.tile_shift[2]) - 1u);
	x = (bx << p.tile_shift[0]) + lx;
	y = (by << p.tile_shift[1]) + ly;
	z = (bz << p.tile_shift[2]) + lz;
}

#endif
