/* das_burst.hip -- the general kernel (das.hip) for an ENSEMBLE: several RF frames of one geometry beamformed by one launch
 * (beamformer_hip_push_data_burst_with_compute; the Flash / ULM use: hundreds of frames from one parameter block).
 *
 * das.hip spends most of its VALU slots per (voxel, channel, transmit) term on work that does not depend on the RF: the lateral
 * distance, the f-number test, the square root, the sample index, its row-end settlement (settle_index, das_exact.h), the cos^2
 * apodization, the tap address, the interpolation weights and the demodulation phasor.  Across an ensemble that work is the same
 * for every frame.  Here a thread owns one voxel of BF_BURST_FRAMES_PER_THREAD frames: it walks das_rca's loops (transmit outer,
 * channel inner -- the single kernel's summation order without its channel split) ONCE, computes the above once per term, and per
 * frame only gathers, interpolates, rotates, weights and accumulates.  The gathers of all frames of a term are issued back to back
 * before the first is consumed (one wait per term, not one per frame): frame f's DAS input lies at rf + f * rf_stride, so they are
 * the same vector offset on FB wave-uniform bases.
 *
 * Grid: x = the general kernel's tiles (DasDecision::general: 256 voxels a block, no channel split -- the frames fill the chip
 * instead), y = groups of FB frames; the last group may hold fewer (a wave-uniform count): its spare frames read the group's last
 * frame again and store nothing, so the loops carry no per-frame branch.
 *
 * The per-frame arithmetic is sample_rf's (das_common.h) and Accumulator's (das_general.h), expression for expression, with the
 * multiply-adds fused by hand and the same way in every frame slot (burst_term).  The ROUNDINGS therefore differ from das.hip's by
 * design: there hipcc contracts as it sees fit, here the fusions are fixed, so a frame of a burst is within float rounding of its
 * single push and not bit-identical to it (measured: none is) -- what is guaranteed instead is that its bits do not depend on its
 * slot.  RCA family
 * only (RCA_TPW, RCA_VLS, Flash): 3 interpolation modes x real / IQ x with / without coherency weighting = 12 instantiations.
 * No LDS, no barrier, no MFMA: gather / VALU bound as das.hip is.
 *
 * das_readi_burst_kernel is the same for a READI SWEEP (beamformer_hip_push_data_readi_sweep_with_compute): the group acquisitions of a
 * READI image, frame f beamformed under row groups[f] of the Hadamard matrix.  das_forces<READI>'s loops (das.hip) walked once, the
 * same grid and frame slots, burst_term with one weight per slot -- the apodization times the slot's sign --: 12 more instantiations.
 *
 * das_burst_views.hip holds das_burst_kernel for an ensemble on several GRIDS; burst_term, which all three share, is das_burst_term.h.
 */
#include "das_burst_term.h"

/* das.glsl:368-407 + :204-231 (das_rca) over FB frames. */
template <int INTERP, bool CPLX, bool CW>
__global__ __launch_bounds__(256) void das_burst_kernel(const BfDasArgs p, const BfBurstArgs q)
{
	const GeneralTile tile = general_tile(p, blockIdx.x);
	if (!tile.valid) return;
	const uint32_t bx = tile.bx, by = tile.by, bz = tile.bz;

	/* (tile_voxel's text, das_general.h, restated: tried behind general_tile with this compiler, the call turned a branch of the range
	 * test below into a select and gave every kernel here other registers) */
	uint32_t tid = threadIdx.x;
	uint32_t lx  = tid & ((1u << p.tile_shift[0]) - 1u);
	uint32_t ly  = (tid >> p.tile_shift[0]) & ((1u << p.tile_shift[1]) - 1u);
	uint32_t lz  = (tid >> (p.tile_shift[0] + p.tile_shift[1])) & ((1u << p.tile_shift[2]) - 1u);
	uint32_t x = (bx << p.tile_shift[0]) + lx;
	uint32_t y = (by << p.tile_shift[1]) + ly;
	uint32_t zl = (bz << p.tile_shift[2]) + lz;       /* z inside the shard */
	if (!(x < p.size[0] && y < p.size[1] && zl < p.z_count)) return;

	/* this block's frames: first .. first + count - 1; the spare slots of a short last group alias its last frame */
	uint32_t first, count;
	burst_frames(q.frame_count, first, count);
	const char *rf[FB];
	for (int f = 0; f < FB; f++) {
		const uint32_t frame = first + ((uint32_t)f < count ? (uint32_t)f : count - 1u);
		rf[f] = (const char *)p.rf + (uint64_t)frame * q.rf_stride;
	}
	Accumulator<CPLX, CW, false> acc[FB];
	for (int f = 0; f < FB; f++) acc[f].init();

	uint32_t z = p.z_first + zl;
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

	const uint64_t out_index = (uint64_t)p.size[0] * p.size[1] * zl + (uint64_t)p.size[0] * y + x;
	for (int f = 0; f < FB; f++) {
		if ((uint32_t)f < count) {
			reinterpret_cast<sample_t<CPLX> *>((char *)p.out + (uint64_t)(first + (uint32_t)f) * q.out_stride)[out_index] = coherency_weighted<CW>(acc[f].coherent, acc[f].incoherent);
		}
	}
}

/* das.glsl:368-407 + :323-366 (READI_FORCES) over FB frames, frame f under row q.groups[f] of the Hadamard matrix: das_forces<READI>
 * (das.hip) in its own loop order -- channel, transmit group, transmit event -- without the channel split, so a frame's sum runs in the
 * single frame's order.  Once per channel: the receive term, the aperture test, the apodization.  Once per term: the transmit term, the
 * row-end settlement and everything burst_term takes once.  Per frame: the gather and the weight apodization * h[f], where
 * h[f] = H[groups[f] * G + tx_group] (binary16 +-1: the product is exact) is block-uniform and read through scalar loads -- the table
 * holds G * G >= 4 halves, an even count, and is read as 32-bit words. */
template <int INTERP, bool CPLX, bool CW>
__global__ __launch_bounds__(256) void das_readi_burst_kernel(const BfDasArgs p, const BfReadiSweepArgs r)
{
	const BfBurstArgs &q = r.burst;
	const GeneralTile tile = general_tile(p, blockIdx.x);
	if (!tile.valid) return;
	const uint32_t bx = tile.bx, by = tile.by, bz = tile.bz;

	/* (tile_voxel's text restated, as in das_burst_kernel) */
	uint32_t tid = threadIdx.x;
	uint32_t lx  = tid & ((1u << p.tile_shift[0]) - 1u);
	uint32_t ly  = (tid >> p.tile_shift[0]) & ((1u << p.tile_shift[1]) - 1u);
	uint32_t lz  = (tid >> (p.tile_shift[0] + p.tile_shift[1])) & ((1u << p.tile_shift[2]) - 1u);
	uint32_t x = (bx << p.tile_shift[0]) + lx;
	uint32_t y = (by << p.tile_shift[1]) + ly;
	uint32_t zl = (bz << p.tile_shift[2]) + lz;       /* z inside the shard */
	if (!(x < p.size[0] && y < p.size[1] && zl < p.z_count)) return;

	/* this block's frames, as in das_burst_kernel; row[f]: where frame f's signs begin in the Hadamard matrix */
	uint32_t first, count;
	burst_frames(q.frame_count, first, count);
	const uint32_t G = p.readi_group_count;
	const char *rf[FB];
	uint32_t row[FB];
	for (int f = 0; f < FB; f++) {
		const uint32_t frame = first + ((uint32_t)f < count ? (uint32_t)f : count - 1u);
		rf[f]  = (const char *)p.rf + (uint64_t)frame * q.rf_stride;
		row[f] = r.groups[frame] * G;
	}
	Accumulator<CPLX, CW, false> acc[FB];
	for (int f = 0; f < FB; f++) acc[f].init();
	const uint32_t *hadamard = reinterpret_cast<const uint32_t *>(p.readi_hadamard);

	uint32_t z = p.z_first + zl;
	/* das.glsl:374-376; the host pre-multiplied the voxel transform: (xx, xy, xz) is in transducer space (das.hip das_forces) */
	float xx, xy, xz;
	voxel_point(p, x, y, z, xx, xy, xz);

	/* das.glsl:323-366 */
	const int S = p.sample_count, A = p.acquisition_count, C = p.channel_count;
	const float z_delta_squared     = xz * xz;
	const float transmit_y_delta    = xy - p.pitch[1] * (float)C * 0.5f;
	const float transmit_yz_squared = transmit_y_delta * transmit_y_delta + z_delta_squared;
	const float f_over_z            = p.f_number * hw_rcp(xz);

	for (int channel = 0; channel < C; channel++) {
		float receive_x_delta = xx - (float)channel * p.pitch[0];
		float a_arg           = __builtin_fabsf(receive_x_delta * f_over_z);
		if (!(a_arg < 0.5f)) continue;

		float receive_index = sample_index(hw_sqrt(receive_x_delta * receive_x_delta + z_delta_squared), p);
		float apodization   = apodize(a_arg);

		const int channel_rf_offset = channel * S * A;
		for (uint32_t tx_group = 0; tx_group < G; tx_group++) {
			int rf_offset = channel_rf_offset;     /* every group's events read the channel's A rows: the groups differ in geometry and sign */
			SlotWeights weights;
			for (int f = 0; f < FB; f++) {
				const uint32_t at   = row[f] + tx_group;
				const uint32_t word = hadamard[at >> 1];
				_Float16 h = __builtin_bit_cast(_Float16, (uint16_t)((at & 1u) ? word >> 16 : word));
				weights.w[f] = apodization * (float)h;
			}
			for (int tx_event = 0; tx_event < A; tx_event++) {
				float tx_element       = (float)tx_group * (float)A + (float)tx_event;
				float transmit_x_delta = xx - p.pitch[0] * tx_element;
				float transmit_index   = div_speed_of_sound(hw_sqrt(transmit_yz_squared + transmit_x_delta * transmit_x_delta) * p.sampling_frequency, p);
				const float index = settle_index<BF_DAS_READI, INTERP>(receive_index + transmit_index, p, x, y, z, channel, (int)tx_group * A + tx_event);
				burst_term<INTERP, CPLX, CW>(rf, rf_offset, index, weights, p, acc);
				rf_offset += S;
			}
		}
	}

	const uint64_t out_index = (uint64_t)p.size[0] * p.size[1] * zl + (uint64_t)p.size[0] * y + x;
	for (int f = 0; f < FB; f++) {
		if ((uint32_t)f < count) {
			reinterpret_cast<sample_t<CPLX> *>((char *)p.out + (uint64_t)(first + (uint32_t)f) * q.out_stride)[out_index] = coherency_weighted<CW>(acc[f].coherent, acc[f].incoherent);
		}
	}
}

/* `a`: the general kernel's arguments without a channel split (DasDecision::general), rf / out those of the burst's first frame. */
extern "C" hipError_t bf_launch_das_burst(const BfDasArgs *a, const BfBurstArgs *b, hipStream_t s)
{
	const uint32_t groups = (b->frame_count + BF_BURST_FRAMES_PER_THREAD - 1u) / BF_BURST_FRAMES_PER_THREAD;
	if (a->family != BF_DAS_RCA || a->split_shift || b->frame_count == 0 || groups > 65535u) return hipErrorInvalidValue;
	return bf_dispatch_kind(a, [&](auto interp, auto cplx, auto cw) {
		hipLaunchKernelGGL((das_burst_kernel<interp, cplx, cw>), dim3(bf_general_grid_blocks(a), groups), dim3(256), 0, s, *a, *b);
		return hipGetLastError();
	});
}

/* `a` as for bf_launch_das_burst, family READI; b->groups: frame_count validated group ids on the device. */
extern "C" hipError_t bf_launch_das_readi_sweep(const BfDasArgs *a, const BfReadiSweepArgs *b, hipStream_t s)
{
	const uint32_t frames = b->burst.frame_count;
	const uint32_t groups = (frames + BF_BURST_FRAMES_PER_THREAD - 1u) / BF_BURST_FRAMES_PER_THREAD;
	if (a->family != BF_DAS_READI || a->split_shift || a->readi_group_count < 2u || !a->readi_hadamard || !b->groups || frames == 0 || groups > 65535u)
		return hipErrorInvalidValue;
	return bf_dispatch_kind(a, [&](auto interp, auto cplx, auto cw) {
		hipLaunchKernelGGL((das_readi_burst_kernel<interp, cplx, cw>), dim3(bf_general_grid_blocks(a), groups), dim3(256), 0, s, *a, *b);
		return hipGetLastError();
	});
}
