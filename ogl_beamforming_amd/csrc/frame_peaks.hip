/* frame_peaks.hip -- the local maxima of several frames of the frame ring in three launches (beamformer_hip_find_peaks_last_frames: the
 * coarse frames of a burst searched where they lie, so that the patches of a ULM refinement can be placed without downloading a frame).
 *
 * DEFINITION (include/ogl_beamformer_hip.h has it for callers; tests/frame_peaks_ref.py is its numpy restatement).  Every decision is
 * taken on ONE float32 a voxel, q: re * re + im * im for a complex frame, every operation rounded on its own (contraction off), fabsf(v)
 * for a real one -- no square root decides anything.  A voxel is finite when q is, eligible when it is finite and q >= t.  A voxel at
 * flat frame index i (x fastest) is a peak when it is eligible, inside the box, and for every voxel n of its 3 x 3 x 3 neighbourhood --
 * clipped to the FRAME, not to the box -- with finite q_n: q > q_n where n's flat index is below i, q >= q_n where it is above.  A
 * frame's list is in ascending flat index.
 *
 * Mark: grid y the frame, grid x the block; a wave owns 64 consecutive x of one box row, waves numbered in flat box order, four a block
 * (a row shorter than a wave leaves lanes idle: nothing is packed, so neither results nor order can depend on packing).  A lane forms
 * its q from one coalesced load; the ballot of the eligible lanes gives above_threshold, and a wave whose ballot is empty is done.
 * Otherwise the nine rows of the neighbourhood: every lane loads the voxel at its own x, x - 1 and x + 1 arrive by wave shuffles, lanes
 * 0 and 63 load their outer neighbour themselves -- a q is formed once a row and lane.  A q that is not finite becomes NaN where it is
 * formed: every comparison with it is false, which is "does not count".  Out: the wave's 64-bit peak ballot and, a block, one word
 * (peaks | eligible << 16, both at most 256).
 * Scan: one block a frame turns those words into exclusive offsets (saturating at 2^32 - 1: only "below the cap" is asked of them) and
 * the frame's found and above_threshold -- integer sums, any order gives the same.
 * Emit: the mark pass's grid.  A block without a peak leaves after one load; a lane whose bit is set has rank offset + the peaks of the
 * block's earlier waves + popcount(mask & lower lanes), and below the cap stores its record at list[first + rank] with two 16-byte
 * stores.  No atomics anywhere: a peak's position in the list is a function of its index.
 *
 * DEPOSIT (beamformer_hip_accumulate_peaks_last_frames: the peaks binned into the localisation map, no list made).  Behind the same mark
 * pass, on its grid: a block without a peak stores a zero word and leaves after one load; a lane whose bit is set forms its record with
 * the emit pass's own functions (magnitude_at and fit_axis: one text for both), places p = index + offset through its frame's 3 x 4 double
 * matrix -- ((A[r][3] + A[r][0] p_x) + A[r][1] p_y) + A[r][2] p_z, contraction off --, bins b_r = floor(m_r + 0.5) and, inside the map,
 * adds 1 to its uint32 count with one returnless integer atomic.  Integer additions commute: the map's bytes are a function of the
 * multiset of deposits -- the one place this file uses an atomic, and no floating-point one.  The ballots of the lanes inside and
 * outside give a block's word (deposited | outside << 16, both at most 256): the scan kernel sums such words as it sums the mark
 * pass's, so a second launch of it makes the per-frame tallies.
 * CONVERT (beamformer_hip_queue_localisation_map): one coalesced pass, count -> (float)count * scale, four voxels a lane. */
#include <hip/hip_runtime.h>
#include "bf_kernels.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

__device__ __forceinline__ bool is_finite(float a) { return (__float_as_uint(a) & 0x7F800000u) != 0x7F800000u; }

/* the decision value of voxel i: finite, or NaN */
__device__ __forceinline__ float decision_at(const float *frame, uint64_t i, uint32_t cplx)
{
	#pragma clang fp contract(off)
	float q;
	if (cplx) { const f32x2 c = ((const f32x2 *)frame)[i]; q = c.x * c.x + c.y * c.y; }
	else q = __builtin_fabsf(frame[i]);
	return is_finite(q) ? q : __builtin_nanf("");
}

/* the frame metrics' magnitude of voxel i (frame_metrics.hip: magnitude_at) */
__device__ __forceinline__ float magnitude_at(const float *frame, uint64_t i, uint32_t cplx)
{
	#pragma clang fp contract(off)
	if (cplx) { const f32x2 c = ((const f32x2 *)frame)[i]; return __builtin_sqrtf(c.x * c.x + c.y * c.y); }
	return __builtin_fabsf(frame[i]);
}

/* where wave w of the row's box lies: its first x in the box, and the box row's y and z in the FRAME */
__device__ __forceinline__ void wave_at(const BfPeaksRow &row, uint32_t w, uint32_t &x0, uint32_t &y, uint32_t &z)
{
	const uint32_t r = w / row.waves_per_row, zb = r / row.count[1];
	x0 = (w - r * row.waves_per_row) * 64u;
	y = row.first[1] + (r - zb * row.count[1]);
	z = row.first[2] + zb;
}

} // namespace

__global__ __launch_bounds__(256) void frame_peaks_mark_kernel(const char *__restrict__ ring, const BfPeaksRow *__restrict__ rows,
                                                               uint64_t *__restrict__ masks, uint32_t *__restrict__ counts)
{
	#pragma clang fp contract(off)
	const BfPeaksRow &row = rows[blockIdx.y];
	if (blockIdx.x >= row.blocks) return;
	const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), w = blockIdx.x * 4u + wave;
	__shared__ uint32_t tallies[4];
	uint32_t tally = 0;
	if (w < row.waves) {
		const float *frame = (const float *)(ring + row.offset);
		const uint32_t cplx = row.cplx, px = row.points[0], py = row.points[1], pz = row.points[2];
		const uint64_t plane = (uint64_t)px * py;
		uint32_t x0, y, z;
		wave_at(row, w, x0, y, z);
		/* lanes past the box but inside the frame load too: their q is the x + 1 neighbour of the lane before them */
		const uint64_t x = (uint64_t)row.first[0] + x0 + lane;
		const bool in_frame = x < px;
		const float nan = __builtin_nanf("");
		const float q = in_frame ? decision_at(frame, z * plane + (uint64_t)y * px + x, cplx) : nan;
		const bool eligible = x0 + lane < row.count[0] && q >= row.threshold;
		const uint64_t above = __ballot(eligible);
		uint64_t peaks = 0;
		if (above) {
			bool beaten = false;
			#pragma unroll
			for (int dz = -1; dz <= 1; dz++) {
				const uint32_t zz = z + (uint32_t)dz;                   /* (z - 1 of plane 0 wraps: not below pz) */
				if (zz >= pz) continue;
				#pragma unroll
				for (int dy = -1; dy <= 1; dy++) {
					const uint32_t yy = y + (uint32_t)dy;
					if (yy >= py) continue;
					const uint64_t at = zz * plane + (uint64_t)yy * px + x;
					const bool centre = dz == 0 && dy == 0, below = dz < 0 || (dz == 0 && dy < 0);
					const float c = centre ? q : (in_frame ? decision_at(frame, at, cplx) : nan);
					float l = __shfl_up(c, 1, 64), r = __shfl_down(c, 1, 64);
					/* (lane 0 lies inside the box, so x - 1 is at most px - 2) */
					if (lane == 0)  l = x >= 1 ? decision_at(frame, at - 1, cplx) : nan;
					if (lane == 63) r = x + 1 < px ? decision_at(frame, at + 1, cplx) : nan;
					if (below)       beaten |= (l >= q) | (c >= q) | (r >= q);
					else if (centre) beaten |= (l >= q) | (r > q);
					else             beaten |= (l > q) | (c > q) | (r > q);
				}
			}
			peaks = __ballot(eligible && !beaten);
		}
		if (lane == 0) masks[row.wave_first + w] = peaks;
		tally = (uint32_t)__popcll(peaks) | (uint32_t)__popcll(above) << 16;
	}
	if (lane == 0) tallies[wave] = tally;
	__syncthreads();
	if (threadIdx.x == 0) counts[row.block_first + blockIdx.x] = tallies[0] + tallies[1] + tallies[2] + tallies[3];
}

__global__ __launch_bounds__(1024) void frame_peaks_scan_kernel(const BfPeaksRow *__restrict__ rows, const uint32_t *__restrict__ counts,
                                                                uint32_t *__restrict__ offsets, BfPeaksResult *__restrict__ results)
{
	const BfPeaksRow &row = rows[blockIdx.x];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	__shared__ uint32_t wave_peaks[16], wave_above[16];
	uint64_t found = 0, above = 0;
	for (uint32_t base = 0; base < row.blocks; base += 1024u) {
		const uint32_t k = base + threadIdx.x, word = k < row.blocks ? counts[row.block_first + k] : 0u;
		const uint32_t mine = word & 0xFFFFu;
		uint32_t upto = mine, eligible = word >> 16;
		for (int off = 1; off < 64; off <<= 1) { const uint32_t v = __shfl_up(upto, off, 64); if (lane >= (uint32_t)off) upto += v; }
		for (int off = 32; off > 0; off >>= 1) eligible += __shfl_xor(eligible, off, 64);
		if (lane == 63) { wave_peaks[wave] = upto; wave_above[wave] = eligible; }
		__syncthreads();
		uint32_t before = 0, all = 0, all_above = 0;
		for (uint32_t j = 0; j < 16; j++) {
			const uint32_t v = wave_peaks[j];
			if (j < wave) before += v;
			all += v; all_above += wave_above[j];
		}
		if (k < row.blocks) {
			const uint64_t first = found + before + (upto - mine);
			offsets[row.block_first + k] = first > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)first;
		}
		found += all; above += all_above;
		__syncthreads();
	}
	if (threadIdx.x == 0) { BfPeaksResult r; r.found = found; r.above_threshold = above; results[blockIdx.x] = r; }
}

namespace {

/* one axis of a record: the voxel `step` before and behind the peak along it, where both lie in the frame (`at` and `points` along the axis) */
__device__ __forceinline__ bool fit_axis(const float *frame, uint32_t cplx, uint64_t i, uint64_t step, uint64_t at, uint32_t points, float m0, float &offset)
{
	#pragma clang fp contract(off)
	offset = 0.0f;
	if (at < 1 || at + 1 >= points) return false;
	const float lo = magnitude_at(frame, i - step, cplx), hi = magnitude_at(frame, i + step, cplx);
	if (!is_finite(lo) || !is_finite(hi)) return false;
	const float den = (lo + hi) - (m0 + m0);
	if (!(den < 0.0f)) return false;
	const float o = 0.5f * (lo - hi) / den;
	offset = o < -0.5f ? -0.5f : o > 0.5f ? 0.5f : o;
	return true;
}

} // namespace

__global__ __launch_bounds__(256) void frame_peaks_emit_kernel(const char *__restrict__ ring, const BfPeaksRow *__restrict__ rows,
                                                               const uint64_t *__restrict__ masks, const uint32_t *__restrict__ counts,
                                                               const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ firsts,
                                                               uint4 *__restrict__ list)
{
	#pragma clang fp contract(off)
	const BfPeaksRow &row = rows[blockIdx.y];
	if (blockIdx.x >= row.blocks) return;
	if ((counts[row.block_first + blockIdx.x] & 0xFFFFu) == 0) return;
	uint32_t rank = offsets[row.block_first + blockIdx.x];
	if (rank >= row.cap) return;
	const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), w = blockIdx.x * 4u + wave;
	if (w >= row.waves) return;
	for (uint32_t k = 0; k < wave; k++) rank += (uint32_t)__popcll(masks[row.wave_first + (w - wave) + k]);   /* (at most 192 + the offset below the cap: no wrap) */
	const uint64_t mask = masks[row.wave_first + w];
	if (!(mask >> lane & 1ull)) return;
	rank += (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
	if (rank >= row.cap) return;

	const float *frame = (const float *)(ring + row.offset);
	const uint32_t cplx = row.cplx, px = row.points[0], py = row.points[1], pz = row.points[2];
	const uint64_t plane = (uint64_t)px * py;
	uint32_t x0, y, z;
	wave_at(row, w, x0, y, z);
	const uint64_t x = (uint64_t)row.first[0] + x0 + lane, i = z * plane + (uint64_t)y * px + x;
	const float m0 = magnitude_at(frame, i, cplx);
	float ox, oy, oz;
	uint32_t fitted = 0;
	if (fit_axis(frame, cplx, i, 1, x, px, m0, ox))     fitted |= 1u;
	if (fit_axis(frame, cplx, i, px, y, py, m0, oy))    fitted |= 2u;
	if (fit_axis(frame, cplx, i, plane, z, pz, m0, oz)) fitted |= 4u;
	uint4 *record = list + 2ull * ((uint64_t)firsts[blockIdx.y] + rank);
	record[0] = make_uint4((uint32_t)x, y, z, __float_as_uint(m0));
	record[1] = make_uint4(__float_as_uint(ox), __float_as_uint(oy), __float_as_uint(oz), fitted);
}

/* ring, rows, masks, counts, offsets, results: device memory; rows[k].wave_first + rows[k].waves masks, rows[k].block_first +
 * rows[k].blocks counts and offsets, frame_count results.  Every row's box lies inside its frame and its frame inside the ring: the
 * caller's business (frame_ops.cpp: find_peaks_last_frames), nothing here re-checks it. */
extern "C" hipError_t bf_launch_frame_peaks_mark(const void *ring, const BfPeaksRow *rows, uint32_t frame_count, uint32_t max_blocks,
                                                 uint64_t *masks, uint32_t *counts, uint32_t *offsets, BfPeaksResult *results, hipStream_t s)
{
	if (!ring || !rows || !masks || !counts || !offsets || !results || frame_count == 0 || frame_count > 65535u || max_blocks == 0 ||
	    max_blocks > BF_PEAKS_MAX_BLOCKS) return hipErrorInvalidValue;
	hipLaunchKernelGGL(frame_peaks_mark_kernel, dim3(max_blocks, frame_count), dim3(256), 0, s, (const char *)ring, rows, masks, counts);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(frame_peaks_scan_kernel, dim3(frame_count), dim3(1024), 0, s, rows, (const uint32_t *)counts, offsets, results);
	return hipGetLastError();
}

/* firsts (device, frame_count): where each frame's records start in `list`; list: room for firsts[k] + min(found, cap) records of every
 * frame k, 16-byte aligned */
extern "C" hipError_t bf_launch_frame_peaks_emit(const void *ring, const BfPeaksRow *rows, uint32_t frame_count, uint32_t max_blocks,
                                                 const uint64_t *masks, const uint32_t *counts, const uint32_t *offsets, const uint32_t *firsts,
                                                 void *list, hipStream_t s)
{
	if (!ring || !rows || !masks || !counts || !offsets || !firsts || !list || ((uintptr_t)list & 15u) || frame_count == 0 || frame_count > 65535u ||
	    max_blocks == 0 || max_blocks > BF_PEAKS_MAX_BLOCKS) return hipErrorInvalidValue;
	hipLaunchKernelGGL(frame_peaks_emit_kernel, dim3(max_blocks, frame_count), dim3(256), 0, s, (const char *)ring, rows, masks, counts, offsets,
	                   firsts, (uint4 *)list);
	return hipGetLastError();
}

/* Deposit: the mark pass's grid.  placements[frame][12]: row-major 3 x 4, double; map: a.points voxels of uint32, x fastest; words: one
 * a block, deposited | outside << 16. */
__global__ __launch_bounds__(256) void localisation_deposit_kernel(const char *__restrict__ ring, const BfPeaksRow *__restrict__ rows,
                                                                  const double *__restrict__ placements, const uint64_t *__restrict__ masks,
                                                                  const uint32_t *__restrict__ counts, BfMapArgs a, uint32_t *__restrict__ map,
                                                                  uint32_t *__restrict__ words)
{
	#pragma clang fp contract(off)
	const BfPeaksRow &row = rows[blockIdx.y];
	if (blockIdx.x >= row.blocks) return;
	if ((counts[row.block_first + blockIdx.x] & 0xFFFFu) == 0) {
		if (threadIdx.x == 0) words[row.block_first + blockIdx.x] = 0u;
		return;
	}
	const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), w = blockIdx.x * 4u + wave;
	__shared__ uint32_t tallies[4];
	uint32_t tally = 0;
	if (w < row.waves) {
		const uint64_t mask = masks[row.wave_first + w];
		const bool mine = mask >> lane & 1ull;
		bool inside = false;
		if (mine) {
			/* the emit pass's record of this voxel, by the emit pass's functions; without offsets no neighbour is read */
			const float *frame = (const float *)(ring + row.offset);
			const uint32_t cplx = row.cplx, nx = row.points[0], ny = row.points[1], nz = row.points[2];
			const uint64_t plane = (uint64_t)nx * ny;
			uint32_t x0, y, z;
			wave_at(row, w, x0, y, z);
			const uint64_t x = (uint64_t)row.first[0] + x0 + lane, i = z * plane + (uint64_t)y * nx + x;
			float ox = 0.0f, oy = 0.0f, oz = 0.0f;
			if (a.use_offsets) {
				const float m0 = magnitude_at(frame, i, cplx);
				(void)fit_axis(frame, cplx, i, 1, x, nx, m0, ox);
				(void)fit_axis(frame, cplx, i, nx, y, ny, m0, oy);
				(void)fit_axis(frame, cplx, i, plane, z, nz, m0, oz);
			}
			const double px = (double)(uint32_t)x + (double)ox, py = (double)y + (double)oy, pz = (double)z + (double)oz;
			const double *A = placements + 12u * blockIdx.y;
			uint32_t bin[3];
			inside = true;
			#pragma unroll
			for (int r = 0; r < 3; r++) {
				const double m = ((A[4 * r + 3] + A[4 * r] * px) + A[4 * r + 1] * py) + A[4 * r + 2] * pz;
				const double b = __builtin_floor(m + 0.5);
				const bool in = b >= 0.0 && b < (double)a.points[r];        /* (NaN: neither) */
				bin[r] = in ? (uint32_t)b : 0u;
				inside &= in;
			}
			/* the one atomic of the file: an integer add whose result nobody reads */
			if (inside) atomicAdd(map + (((uint64_t)bin[2] * a.points[1] + bin[1]) * a.points[0] + bin[0]), 1u);
		}
		const uint64_t deposited = __ballot(inside), outside = __ballot(mine && !inside);
		tally = (uint32_t)__popcll(deposited) | (uint32_t)__popcll(outside) << 16;
	}
	if (lane == 0) tallies[wave] = tally;
	__syncthreads();
	if (threadIdx.x == 0) words[row.block_first + blockIdx.x] = tallies[0] + tallies[1] + tallies[2] + tallies[3];
}

/* Convert: out[i] = (float)map[i] * scale -- one conversion rounded to nearest, one float32 multiply.  The first `quads` groups of four
 * voxels go as 16 bytes a lane, the voxels behind them one a lane. */
__global__ __launch_bounds__(256) void localisation_convert_kernel(const uint32_t *__restrict__ map, float *__restrict__ out, uint64_t voxels,
                                                           uint64_t quads, float scale)
{
	#pragma clang fp contract(off)
	const uint64_t stride = (uint64_t)gridDim.x * 256u, t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
	for (uint64_t k = t; k < quads; k += stride) {
		const uint4 c = ((const uint4 *)map)[k];
		((float4 *)out)[k] = make_float4((float)c.x * scale, (float)c.y * scale, (float)c.z * scale, (float)c.w * scale);
	}
	for (uint64_t i = 4u * quads + t; i < voxels; i += stride) out[i] = (float)map[i] * scale;
}

/* Behind bf_launch_frame_peaks_mark on the same stream and tables.  placements: frame_count x 12 doubles; map: the product of a->points
 * uint32 (at most 2^28); words: a uint32 a block, as counts; tallies[frame]: found = deposited, above_threshold = outside -- the scan
 * kernel over `words`, which rewrites `offsets` (nothing reads them behind the deposit).  All device memory. */
extern "C" hipError_t bf_launch_localisation_deposit(const void *ring, const BfPeaksRow *rows, const double *placements, uint32_t frame_count,
                                                    uint32_t max_blocks, const uint64_t *masks, const uint32_t *counts, uint32_t *offsets,
                                                    const BfMapArgs *a, uint32_t *map, uint32_t *words, BfPeaksResult *tallies, hipStream_t s)
{
	if (!ring || !rows || !placements || !masks || !counts || !offsets || !a || !map || !words || !tallies || frame_count == 0 ||
	    frame_count > 65535u || max_blocks == 0 || max_blocks > BF_PEAKS_MAX_BLOCKS) return hipErrorInvalidValue;
	if (!a->points[0] || !a->points[1] || !a->points[2] || (uint64_t)a->points[0] * a->points[1] > BF_MAP_MAX_VOXELS ||
	    (uint64_t)a->points[0] * a->points[1] * a->points[2] > BF_MAP_MAX_VOXELS) return hipErrorInvalidValue;
	hipLaunchKernelGGL(localisation_deposit_kernel, dim3(max_blocks, frame_count), dim3(256), 0, s, (const char *)ring, rows, placements, masks,
	                   counts, *a, map, words);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(frame_peaks_scan_kernel, dim3(frame_count), dim3(1024), 0, s, rows, (const uint32_t *)words, offsets, tallies);
	return hipGetLastError();
}

/* map: `voxels` uint32; out: `voxels` floats (a frame of the ring); both device memory */
extern "C" hipError_t bf_launch_localisation_convert(const uint32_t *map, float *out, uint64_t voxels, float scale, hipStream_t s)
{
	if (!map || !out || voxels == 0 || voxels > BF_MAP_MAX_VOXELS) return hipErrorInvalidValue;
	const uint64_t quads = (((uintptr_t)map | (uintptr_t)out) & 15u) ? 0u : voxels / 4u;
	const uint64_t lanes = quads ? quads : voxels, blocks = (lanes + 255u) / 256u;
	hipLaunchKernelGGL(localisation_convert_kernel, dim3((uint32_t)(blocks < 4096u ? blocks : 4096u)), dim3(256), 0, s, map, out, voxels, quads, scale);
	return hipGetLastError();
}
