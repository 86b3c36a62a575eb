/* frame_tracks.hip -- the peaks of consecutive frames of the frame ring linked into pairs (beamformer_hip_pair_peaks_last_frames: the
 * velocity map of ULM and the rejection of detections that do not persist, without a peak list leaving the device), the pairs chained
 * into tracks and kept by length (beamformer_hip_track_peaks_last_frames: the chain kernels have their own comment further down), the
 * kept tracks smoothed and drawn into both maps (beamformer_hip_draw_tracks_last_frames: likewise), and the track map's frame
 * (beamformer_hip_queue_track_map).
 *
 * DEFINITION (include/ogl_beamformer_hip.h has it for callers; tests/tracks_ref.py is its numpy restatement).  A frame's peaks are the
 * records frame_peaks.hip emits (the caller runs its mark, scan and emit passes in front of these launches); a peak's rank is its place
 * in that list.  Its position is p = index + offset (the offset dropped without offsets), its map coordinate
 * m_r = ((A[r][3] + A[r][0] p_x) + A[r][1] p_y) + A[r][2] p_z under its frame's 3 x 4 double placement -- the localisation map's
 * formula --; a peak with an m_r that is not finite is unplaced.  For a in frame n and b in frame n + 1: d_r = m_r(b) - m_r(a),
 * d2 = ((d_x d_x) + (d_y d_y)) + (d_z d_z), b within reach of a when d2 <= R2.  f(a): the b within reach of the least (d2, rank of b);
 * g(b): the a within reach of the least (d2, rank of a); (a, b) is a pair when f(a) = b and g(b) = a.  Everything is double arithmetic
 * with contraction off, one expression for both directions.
 *
 * Place: grid y the frame, grid x blocks of 256 records; a lane reads its record's index and offset (32 bytes) and stores three doubles,
 * NaN all three for an unplaced peak; a wave adds the count of its unplaced lanes to the frame's tally with one integer atomic.
 * Nearest, the hot kernel: grid x blocks of 256 queries, grid y the frame pair, grid z the direction (0: f, the queries are frame n's;
 * 1: g, they are frame n + 1's).  A lane owns one query.  The other frame's positions pass through LDS in tiles of 256, stored as three
 * rows of doubles: in the inner loop every lane reads the same address, which LDS serves as a broadcast, without bank conflicts.  A
 * candidate costs three subtractions, three products and two sums in double; the best (d2, rank) is kept with a strict < while the
 * ranks ascend, which is the lexicographic minimum.  A NaN coordinate on either side makes d2 NaN, and every comparison with it false:
 * an unplaced peak neither chooses nor is chosen.  Blocks past their frame's peak count leave at once.  The cost is P_n x P_{n+1}
 * distance evaluations a direction a frame pair: there is no search window.
 * Match, scan, emit: the pair list WITHOUT atomics.  Match: grid x blocks of 256 a, grid y the frame pair; the ballot of the lanes with
 * f(a) = b and g(b) = a is the wave's 64-bit mask, their number a block's word, and a wave adds it to the frame pair's tally (an
 * integer atomic on a counter: the count, not a place).  Scan: one block turns the words of all frame pairs, in frame-pair order,
 * into exclusive offsets -- the lists are packed one behind the other, so one running offset serves them all.  Emit: the match pass's
 * grid; a lane whose bit is set has the place offset + the pairs of the block's earlier waves + popcount(mask & lower lanes): a pair's
 * place is a function of a.  It forms d_r and d2 again (the same expression: the same bits), and with `deposit` the midpoint
 * c_r = 0.5 * (m_r(a) + m_r(b)), its bin floor(c_r + 0.5) and, inside the track map, adds 1 to the bin's uint32 count and
 * q_r = (int64)floor(d_r * 2^20 + 0.5) to its three int64 sums: returnless integer atomics, which commute -- the map's bytes are a
 * function of the multiset of deposits, and there is still no floating-point atomic in the library.  The ballots of the lanes inside and
 * outside go to the frame pair's tally.
 * Convert (beamformer_hip_queue_track_map): one coalesced pass, a voxel a lane. */
#include <hip/hip_runtime.h>
#include "bf_kernels.h"

namespace {

__device__ __forceinline__ bool is_finite(double a) { return (__double_as_longlong(a) & 0x7FF0000000000000ll) != 0x7FF0000000000000ll; }

} // namespace

__global__ __launch_bounds__(256) void tracks_place_kernel(const uint4 *__restrict__ list, const double *__restrict__ placements,
                                                           const uint32_t *__restrict__ firsts, const uint32_t *__restrict__ stored,
                                                           uint32_t use_offsets, double *__restrict__ positions, uint32_t *__restrict__ unplaced)
{
	#pragma clang fp contract(off)
	const uint32_t frame = blockIdx.y, n = stored[frame], k = blockIdx.x * 256u + threadIdx.x;
	if (blockIdx.x * 256u >= n) return;
	bool lost = false;
	if (k < n) {
		const uint64_t at = (uint64_t)firsts[frame] + k;
		const uint4 where = list[2u * at], fit = list[2u * at + 1u];
		const double ox = use_offsets ? (double)__uint_as_float(fit.x) : 0.0, oy = use_offsets ? (double)__uint_as_float(fit.y) : 0.0,
		             oz = use_offsets ? (double)__uint_as_float(fit.z) : 0.0;
		const double px = (double)where.x + ox, py = (double)where.y + oy, pz = (double)where.z + oz;
		const double *A = placements + 12u * frame;
		double m[3];
		bool placed = true;
		#pragma unroll
		for (int r = 0; r < 3; r++) {
			m[r] = ((A[4 * r + 3] + A[4 * r] * px) + A[4 * r + 1] * py) + A[4 * r + 2] * pz;
			placed &= is_finite(m[r]);
		}
		lost = !placed;
		const double nan = __builtin_nan("");
		#pragma unroll
		for (int r = 0; r < 3; r++) positions[3u * at + r] = placed ? m[r] : nan;
	}
	const uint64_t lost_lanes = __ballot(lost);
	if ((threadIdx.x & 63u) == 0 && lost_lanes) atomicAdd(unplaced + frame, (unsigned int)__popcll(lost_lanes));
}

__global__ __launch_bounds__(256) void tracks_nearest_kernel(const double *__restrict__ positions, const uint32_t *__restrict__ firsts,
                                                             const uint32_t *__restrict__ stored, double r2, uint32_t *__restrict__ forward,
                                                             uint32_t *__restrict__ backward)
{
	#pragma clang fp contract(off)
	const uint32_t pair = blockIdx.y, back = blockIdx.z;
	const uint32_t mine = pair + back, other = pair + 1u - back;             /* the queries' frame, the candidates' */
	const uint32_t queries = stored[mine], candidates = stored[other];
	if (blockIdx.x * 256u >= queries) return;
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	const bool live = k < queries;
	const double *q = positions + 3ull * ((uint64_t)firsts[mine] + (live ? k : 0u));
	const double qx = q[0], qy = q[1], qz = q[2];
	const double *from = positions + 3ull * firsts[other];
	__shared__ double tile[3][256];
	double best = __builtin_inf();
	uint32_t best_rank = BF_TRACK_NONE;
	for (uint32_t base = 0; base < candidates; base += 256u) {
		const uint32_t c = base + threadIdx.x, here = candidates - base < 256u ? candidates - base : 256u;
		if (c < candidates) {
			tile[0][threadIdx.x] = from[3ull * c];
			tile[1][threadIdx.x] = from[3ull * c + 1u];
			tile[2][threadIdx.x] = from[3ull * c + 2u];
		}
		__syncthreads();
		#pragma unroll 4
		for (uint32_t j = 0; j < here; j++) {
			/* d = m(b) - m(a) on the way forward and its negative on the way back: a difference and its negative round alike, and a
			 * product does not see the sign, so d2 has the bits of the one expression in both directions */
			const double dx = tile[0][j] - qx, dy = tile[1][j] - qy, dz = tile[2][j] - qz;
			const double d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
			if (d2 <= r2 && d2 < best) { best = d2; best_rank = base + j; }
		}
		__syncthreads();
	}
	if (live) (back ? backward : forward)[(uint64_t)firsts[mine] + k] = best_rank;
}

namespace {

/* is lane a's peak half of a pair, and with which b */
__device__ __forceinline__ bool mutual(const uint32_t *forward, const uint32_t *backward, uint32_t first_a, uint32_t first_b, uint32_t a, uint32_t &b)
{
	b = forward[(uint64_t)first_a + a];
	return b != BF_TRACK_NONE && backward[(uint64_t)first_b + b] == a;
}

} // namespace

__global__ __launch_bounds__(256) void tracks_match_kernel(const uint32_t *__restrict__ firsts, const uint32_t *__restrict__ stored,
                                                           const uint32_t *__restrict__ block_firsts, const uint32_t *__restrict__ forward,
                                                           const uint32_t *__restrict__ backward, uint64_t *__restrict__ masks,
                                                           uint32_t *__restrict__ words, BfTrackTally *__restrict__ tallies)
{
	const uint32_t pair = blockIdx.y, n = stored[pair], a = blockIdx.x * 256u + threadIdx.x;
	if (blockIdx.x * 256u >= n) return;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, block = block_firsts[pair] + blockIdx.x;
	__shared__ uint32_t counts[4];
	uint32_t b = 0;
	const uint64_t mask = __ballot(a < n && mutual(forward, backward, firsts[pair], firsts[pair + 1u], a, b));
	if (lane == 0) {
		masks[4ull * block + wave] = mask;
		counts[wave] = (uint32_t)__popcll(mask);
		if (mask) atomicAdd(&tallies[pair].pairs, (unsigned int)__popcll(mask));
	}
	__syncthreads();
	if (threadIdx.x == 0) words[block] = counts[0] + counts[1] + counts[2] + counts[3];
}

/* one block: words[blocks] (each at most 256, at most 2^26 in all) -> their exclusive offsets */
__global__ __launch_bounds__(1024) void tracks_scan_kernel(const uint32_t *__restrict__ words, uint32_t blocks, uint32_t *__restrict__ offsets)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	__shared__ uint32_t wave_sums[16];
	uint32_t running = 0;
	for (uint32_t base = 0; base < blocks; base += 1024u) {
		const uint32_t k = base + threadIdx.x, mine = k < blocks ? words[k] : 0u;
		uint32_t upto = mine;
		for (int off = 1; off < 64; off <<= 1) { const uint32_t v = __shfl_up(upto, off, 64); if (lane >= (uint32_t)off) upto += v; }
		if (lane == 63) wave_sums[wave] = upto;
		__syncthreads();
		uint32_t before = 0, all = 0;
		for (uint32_t j = 0; j < 16; j++) {
			const uint32_t v = wave_sums[j];
			if (j < wave) before += v;
			all += v;
		}
		if (k < blocks) offsets[k] = running + before + (upto - mine);
		running += all;
		__syncthreads();
	}
}

__global__ __launch_bounds__(256) void tracks_emit_kernel(const double *__restrict__ positions, const uint32_t *__restrict__ firsts,
                                                          const uint32_t *__restrict__ stored, const uint32_t *__restrict__ block_firsts,
                                                          const uint32_t *__restrict__ forward, const uint64_t *__restrict__ masks,
                                                          const uint32_t *__restrict__ words, const uint32_t *__restrict__ offsets, BfTrackArgs t,
                                                          uint32_t *__restrict__ map_counts, unsigned long long *__restrict__ map_sums,
                                                          uint4 *__restrict__ pairs, BfTrackTally *__restrict__ tallies)
{
	#pragma clang fp contract(off)
	const uint32_t pair = blockIdx.y, n = stored[pair];
	if (blockIdx.x * 256u >= n) return;
	const uint32_t block = block_firsts[pair] + blockIdx.x;
	if (words[block] == 0) return;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, a = blockIdx.x * 256u + threadIdx.x;
	uint32_t place = offsets[block];
	for (uint32_t k = 0; k < wave; k++) place += (uint32_t)__popcll(masks[4ull * block + k]);
	const uint64_t mask = masks[4ull * block + wave];
	if (!mask) return;                                                   /* (the whole wave: the ballots below are the wave's own) */
	const bool mine = mask >> lane & 1ull;
	bool inside = false;
	if (mine) {
		place += (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
		const uint32_t b = forward[(uint64_t)firsts[pair] + a];
		const double *ma = positions + 3ull * ((uint64_t)firsts[pair] + a), *mb = positions + 3ull * ((uint64_t)firsts[pair + 1u] + b);
		double d[3], c[3];
		#pragma unroll
		for (int r = 0; r < 3; r++) { const double u = ma[r], v = mb[r]; d[r] = v - u; c[r] = 0.5 * (u + v); }
		const double d2 = ((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2]);
		if (t.deposit) {
			uint32_t bin[3];
			inside = true;
			#pragma unroll
			for (int r = 0; r < 3; r++) {
				const double at = __builtin_floor(c[r] + 0.5);
				const bool in = at >= 0.0 && at < (double)t.points[r];
				bin[r] = in ? (uint32_t)at : 0u;
				inside &= in;
			}
			if (inside) {
				/* integer adds whose results nobody reads; |d_r| <= 2^20 (d2 <= R2 <= 2^40): q_r fits easily */
				const uint64_t voxels = (uint64_t)t.points[0] * t.points[1] * t.points[2];
				const uint64_t at = ((uint64_t)bin[2] * t.points[1] + bin[1]) * t.points[0] + bin[0];
				atomicAdd(map_counts + at, 1u);
				#pragma unroll
				for (int r = 0; r < 3; r++) {
					const long long q = (long long)__builtin_floor(d[r] * BF_TRACK_FIXED + 0.5);
					atomicAdd(map_sums + r * voxels + at, (unsigned long long)q);
				}
			}
		}
		if (pairs) {
			uint4 *record = pairs + 3ull * place;
			const uint64_t dx = (uint64_t)__double_as_longlong(d[0]), dy = (uint64_t)__double_as_longlong(d[1]),
			               dz = (uint64_t)__double_as_longlong(d[2]), dd = (uint64_t)__double_as_longlong(d2);
			record[0] = make_uint4(pair, a, b, inside ? 1u : 0u);
			record[1] = make_uint4((uint32_t)dx, (uint32_t)(dx >> 32), (uint32_t)dy, (uint32_t)(dy >> 32));
			record[2] = make_uint4((uint32_t)dz, (uint32_t)(dz >> 32), (uint32_t)dd, (uint32_t)(dd >> 32));
		}
	}
	if (t.deposit) {
		const uint64_t in = __ballot(inside), out = __ballot(mine && !inside);
		if (lane == 0) {
			if (in)  atomicAdd(&tallies[pair].deposited, (unsigned int)__popcll(in));
			if (out) atomicAdd(&tallies[pair].outside, (unsigned int)__popcll(out));
		}
	}
}

/* Convert: n = counts[i]; below max(1, min_pairs): 0.  Components 0..2: (float)(((double)sum_r / 2^20) / (double)n) * scale -- two double
 * divisions, one conversion rounded to nearest, one float32 multiply; 3: (float)n * scale; 4: (float)((mx mx + my my) + mz mz) * scale
 * with the three means in double. */
__global__ __launch_bounds__(256) void tracks_convert_kernel(const uint32_t *__restrict__ counts, const long long *__restrict__ sums,
                                                             float *__restrict__ out, uint64_t voxels, uint32_t component, uint32_t least, float scale)
{
	#pragma clang fp contract(off)
	const uint64_t stride = (uint64_t)gridDim.x * 256u;
	for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < voxels; i += stride) {
		const uint32_t n = counts[i];
		float v = 0.0f;
		if (n >= least) {
			if (component == 3u) v = (float)n * scale;
			else if (component < 3u) v = (float)(((double)sums[component * voxels + i] / BF_TRACK_FIXED) / (double)n) * scale;
			else {
				const double mx = ((double)sums[i] / BF_TRACK_FIXED) / (double)n, my = ((double)sums[voxels + i] / BF_TRACK_FIXED) / (double)n,
				             mz = ((double)sums[2u * voxels + i] / BF_TRACK_FIXED) / (double)n;
				v = (float)((mx * mx + my * my) + mz * mz) * scale;
			}
		}
		out[i] = v;
	}
}

/* ---- the pairs chained into tracks (beamformer_hip_track_peaks_last_frames).  A record's GLOBAL index is i = firsts[frame] + rank: the
 * lists are packed frame after frame, so ascending i is ascending (frame, rank), the ORDER of the definition.
 * Link: a lane a record; from forward[] and backward[] it forms next[i] -- the mutual partner in the newer frame, or NONE -- and the
 * pair (anc, pos): the mutual partner in the older frame and 1, or i itself and 0 for a head; an unplaced peak (a NaN coordinate)
 * carries anc = NONE and takes part in nothing.
 * Jump: pointer jumping, R = ceil(log2(frames)) launches over all records, from one buffer into the other and never in place:
 * (anc, pos)'[i] = (anc[anc[i]], pos[i] + pos[anc[i]]), one 8-byte gather a record a round.  A chain is at most frames - 1 < 2^R links
 * deep, so after R rounds anc is the head and pos the place in the track -- instead of walking a chain head by head, up to 1023
 * dependent loads on one lane.  The LAST round also lets the tails (next == NONE) store length[head] = pos + 1 and tail_of[head] = i:
 * one writer a head, no atomic; a launch of its own would read (anc, pos) once more for nothing.
 * Keep: blocks of 256 records in global order.  A kept head (anc == i, length >= min_length) gets its number among the block's kept
 * heads (a ballot) and the sum of their lengths before it (a scan), every other record NONE for a number; the block's two totals -- at most 256, and at most 2^18 -- go
 * through tracks_scan_kernel, launched twice.
 * Finish: grid y the frame, so that a wave's ballots are one frame's.  Every record whose head has a number: its track is that number
 * plus its block's offset, its place first_of[head] + pos -- both functions of the records alone, no atomic decides a place --; it
 * stores its 40-byte record, deposits its point by the localisation map's BIN rule and its link by tracks_emit_kernel's expressions
 * (contraction off), and a head stores the 48-byte track record as well.  One kernel instead of a heads pass and a points pass: a head
 * is a point, both read the same tables, and the heads pass would only have stored two words for the points pass to load again.
 * The per-frame tallies: ballots, one integer atomic a wave a counter -- counts, never places. */
namespace {

struct ChainTrack { uint32_t frame, rank, length, first, flags, reserved; double displacement[3]; };
struct ChainPoint { uint32_t track, frame, rank, deposited; double position[3]; };
static_assert(sizeof(ChainTrack) == 48 && sizeof(ChainPoint) == 40, "BeamformerHipPeakTrack's and BeamformerHipTrackPoint's layout");

} // namespace

__global__ __launch_bounds__(256) void tracks_link_kernel(const double *__restrict__ positions, const uint32_t *__restrict__ firsts,
                                                          const uint32_t *__restrict__ stored, uint32_t frames,
                                                          const uint32_t *__restrict__ forward, const uint32_t *__restrict__ backward,
                                                          uint32_t *__restrict__ next, uint2 *__restrict__ links, uint32_t *__restrict__ lengths)
{
	const uint32_t frame = blockIdx.y, n = stored[frame], k = blockIdx.x * 256u + threadIdx.x;
	if (k >= n) return;
	const uint32_t i = firsts[frame] + k;
	uint32_t newer = BF_TRACK_NONE, anc = BF_TRACK_NONE, pos = 0;
	if (is_finite(positions[3ull * i])) {                                /* (an unplaced peak: NaN all three) */
		anc = i;
		if (forward && frame + 1u < frames) {
			const uint32_t first_b = firsts[frame + 1u], b = forward[i];
			if (b != BF_TRACK_NONE && backward[(uint64_t)first_b + b] == k) newer = first_b + b;
		}
		if (forward && frame) {
			const uint32_t first_a = firsts[frame - 1u], a = backward[i];
			if (a != BF_TRACK_NONE && forward[(uint64_t)first_a + a] == k) { anc = first_a + a; pos = 1u; }
		}
	}
	next[i] = newer;
	links[i] = make_uint2(anc, pos);
	lengths[i] = 0;                                                      /* (a head's is stored by its tail, behind the last jump) */
}

__global__ __launch_bounds__(256) void tracks_jump_kernel(const uint2 *__restrict__ in, uint2 *__restrict__ out, uint32_t total,
                                                          const uint32_t *__restrict__ next, uint32_t last, uint32_t *__restrict__ lengths,
                                                          uint32_t *__restrict__ tails)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= total) return;
	uint2 me = in[i];
	if (me.x != BF_TRACK_NONE && me.x != i) {
		const uint2 up = in[me.x];
		me = make_uint2(up.x, me.y + up.y);
	}
	out[i] = me;
	if (last && me.x != BF_TRACK_NONE && next[i] == BF_TRACK_NONE) { lengths[me.x] = me.y + 1u; tails[me.x] = i; }
}

__global__ __launch_bounds__(256) void tracks_keep_kernel(const uint2 *__restrict__ links, const uint32_t *__restrict__ lengths, uint32_t total,
                                                          uint32_t min_length, uint32_t *__restrict__ track_of, uint32_t *__restrict__ first_of,
                                                          uint32_t *__restrict__ track_words, uint32_t *__restrict__ point_words)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t length = 0;
	if (i < total && links[i].x == i) length = lengths[i];
	const bool kept = length && length >= min_length;
	if (!kept) length = 0;
	const uint64_t mask = __ballot(kept);
	uint32_t upto = length;
	for (int off = 1; off < 64; off <<= 1) { const uint32_t v = __shfl_up(upto, off, 64); if (lane >= (uint32_t)off) upto += v; }
	__shared__ uint32_t wave_tracks[4], wave_points[4];
	if (lane == 63) { wave_tracks[wave] = (uint32_t)__popcll(mask); wave_points[wave] = upto; }
	__syncthreads();
	uint32_t tracks_before = 0, points_before = 0, all_tracks = 0, all_points = 0;
	for (uint32_t j = 0; j < 4; j++) {
		const uint32_t t = wave_tracks[j], p = wave_points[j];
		if (j < wave) { tracks_before += t; points_before += p; }
		all_tracks += t; all_points += p;
	}
	/* track_of says for EVERY record whether it is a kept head: the one place where a length meets min_length */
	if (i < total) track_of[i] = kept ? tracks_before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)) : BF_TRACK_NONE;
	if (kept) first_of[i] = points_before + (upto - length);
	if (threadIdx.x == 0) { track_words[blockIdx.x] = all_tracks; point_words[blockIdx.x] = all_points; }
}

__global__ __launch_bounds__(256) void tracks_finish_kernel(const double *__restrict__ positions, const uint32_t *__restrict__ firsts,
                                                            const uint32_t *__restrict__ stored, uint32_t frames, const uint2 *__restrict__ links,
                                                            const uint32_t *__restrict__ next, const uint32_t *__restrict__ lengths,
                                                            const uint32_t *__restrict__ tails, const uint32_t *__restrict__ track_of,
                                                            const uint32_t *__restrict__ first_of, const uint32_t *__restrict__ track_offsets,
                                                            const uint32_t *__restrict__ point_offsets, BfChainArgs t, uint32_t *__restrict__ point_map,
                                                            uint32_t *__restrict__ map_counts, unsigned long long *__restrict__ map_sums,
                                                            ChainTrack *__restrict__ tracks, ChainPoint *__restrict__ points,
                                                            BfChainTally *__restrict__ tallies)
{
	#pragma clang fp contract(off)
	const uint32_t frame = blockIdx.y, n = stored[frame], k = blockIdx.x * 256u + threadIdx.x;
	if (blockIdx.x * 256u >= n) return;
	bool head = false, kept = false, linked = false, point_in = false, link_in = false;
	if (k < n) {
		const uint32_t i = firsts[frame] + k;
		const uint2 me = links[i];
		if (me.x != BF_TRACK_NONE) {
			const uint32_t h = me.x, number = track_of[h];
			head = h == i;
			kept = number != BF_TRACK_NONE;
			if (kept) {
				const uint32_t length = lengths[h], track = track_offsets[h >> 8] + number, place = point_offsets[h >> 8] + first_of[h] + me.y, newer = next[i];
				linked = newer != BF_TRACK_NONE;
				const double *m = positions + 3ull * i;
				const double u[3] = {m[0], m[1], m[2]};
				if (t.deposit & BF_CHAIN_POINTS) {
					/* the localisation map's BIN rule (frame_peaks.hip), on the coordinate the place pass formed by its formula */
					uint32_t bin[3];
					point_in = true;
					#pragma unroll
					for (int r = 0; r < 3; r++) {
						const double b = __builtin_floor(u[r] + 0.5);
						const bool in = b >= 0.0 && b < (double)t.point_map[r];
						bin[r] = in ? (uint32_t)b : 0u;
						point_in &= in;
					}
					if (point_in) atomicAdd(point_map + (((uint64_t)bin[2] * t.point_map[1] + bin[1]) * t.point_map[0] + bin[0]), 1u);
				}
				if (linked && (t.deposit & BF_CHAIN_LINKS)) {
					/* tracks_emit_kernel's deposit, expression for expression */
					const double *mb = positions + 3ull * newer;
					double d[3], c[3];
					#pragma unroll
					for (int r = 0; r < 3; r++) { const double v = mb[r]; d[r] = v - u[r]; c[r] = 0.5 * (u[r] + v); }
					uint32_t bin[3];
					link_in = true;
					#pragma unroll
					for (int r = 0; r < 3; r++) {
						const double at = __builtin_floor(c[r] + 0.5);
						const bool in = at >= 0.0 && at < (double)t.track_map[r];
						bin[r] = in ? (uint32_t)at : 0u;
						link_in &= in;
					}
					if (link_in) {
						const uint64_t voxels = (uint64_t)t.track_map[0] * t.track_map[1] * t.track_map[2];
						const uint64_t at = ((uint64_t)bin[2] * t.track_map[1] + bin[1]) * t.track_map[0] + bin[0];
						atomicAdd(map_counts + at, 1u);
						#pragma unroll
						for (int r = 0; r < 3; r++) {
							const long long q = (long long)__builtin_floor(d[r] * BF_TRACK_FIXED + 0.5);
							atomicAdd(map_sums + r * voxels + at, (unsigned long long)q);
						}
					}
				}
				if (points) {
					ChainPoint &p = points[place];
					p.track = track; p.frame = frame; p.rank = k; p.deposited = (point_in ? 1u : 0u) | (link_in ? 2u : 0u);
					p.position[0] = u[0]; p.position[1] = u[1]; p.position[2] = u[2];
				}
				if (head && tracks) {
					const double *mt = positions + 3ull * tails[h];
					ChainTrack &r = tracks[track];
					r.frame = frame; r.rank = k; r.length = length; r.first = place;
					r.flags = (frame == 0 ? 1u : 0u) | (frame + length == frames ? 2u : 0u); r.reserved = 0;
					r.displacement[0] = mt[0] - u[0]; r.displacement[1] = mt[1] - u[1]; r.displacement[2] = mt[2] - u[2];
				}
			}
		}
	}
	const bool with_points = kept && (t.deposit & BF_CHAIN_POINTS), with_links = kept && linked && (t.deposit & BF_CHAIN_LINKS);
	const uint64_t lanes[8] = {__ballot(head), __ballot(head && kept), __ballot(kept), __ballot(kept && linked), __ballot(point_in),
	                           __ballot(with_points && !point_in), __ballot(link_in), __ballot(with_links && !link_in)};
	if ((threadIdx.x & 63u) == 0) {
		uint32_t *tally = (uint32_t *)(tallies + frame);                 /* (eight counters, in the ballots' order) */
		#pragma unroll
		for (int c = 0; c < 8; c++) if (lanes[c]) atomicAdd(tally + c, (unsigned int)__popcll(lanes[c]));
	}
}

/* ---- the kept tracks drawn into both maps at map resolution (beamformer_hip_draw_tracks_last_frames; the header has the DEFINITION,
 * tests/track_draw_ref.py its numpy restatement).  Both kernels read the finish pass's packed point list where it lies.
 * Smooth: a lane a packed point slot p below the kept total, which it reads from the keep pass's last block (offset + word).  Its
 * track's `first` and `length` bound the window: the sum runs over the track's own run, oldest first, one addition at a time, then one
 * division; three doubles go to smoothed[3 p].  Not launched for w = 0: the draw pass then reads the positions in the point records.
 * Draw: the finish pass's grid -- grid y the frame, so that a wave's tallies are one frame's, grid x blocks of 256 records --, a lane a
 * record.  A record that is a kept point with a successor owns link i = its place in the track: the lane forms d and S, then walks the
 * samples k = 0 .. S - 1 in a loop and carries the B of the sample before in registers; only for k = 0 does it form the predecessor
 * itself, the last sample of link i - 1 from that link's own s, d and S -- eleven double operations a link instead of a scan over
 * samples whose number only the device knows.  A drawn sample costs one integer atomic (POINTS) and four (LINKS), all returnless.  A
 * group of 16 lanes a link striding k was measured against this and was slower where it matters: sixteen times the waves,
 * each with its own tally atomics, for links of 8 samples.  Tallies: every lane counts its own, six shuffle rounds add a wave's, one
 * integer atomic a wave a counter that is not zero. */
namespace {

/* link `slot` -> `slot` + 1 of the packed list: a = s_i, d = s_{i+1} - s_i, S; false: SKIPPED (!(e <= 4096), a NaN included) */
__device__ __forceinline__ bool draw_link(const double *src, uint32_t stride, uint32_t slot, double a[3], double d[3], uint32_t &S)
{
	#pragma clang fp contract(off)
	bool ok = true;
	double e = 0.0;
	#pragma unroll
	for (int r = 0; r < 3; r++) {
		const double u = src[(uint64_t)slot * stride + r], v = src[((uint64_t)slot + 1u) * stride + r];
		a[r] = u; d[r] = v - u;
		const double m = __builtin_fabs(d[r]);
		ok &= m <= BF_DRAW_MAX_SAMPLES;
		e = m > e ? m : e;
	}
	const uint32_t up = ok ? (uint32_t)__builtin_ceil(e) : 0u;
	S = up ? up : 1u;
	return ok;
}

/* B of sample k of a link: floor(c_r + 0.5), c_r = s_r + d_r * t, t = (k + 0.5) / S */
__device__ __forceinline__ void draw_bin(const double a[3], const double d[3], uint32_t S, uint32_t k, double B[3])
{
	#pragma clang fp contract(off)
	const double t = ((double)k + 0.5) / (double)S;
	#pragma unroll
	for (int r = 0; r < 3; r++) {
		const double step = d[r] * t, c = a[r] + step;
		B[r] = __builtin_floor(c + 0.5);
	}
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
	for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off, 64);
	return v;
}

} // namespace

__global__ __launch_bounds__(256) void tracks_smooth_kernel(const ChainTrack *__restrict__ tracks, const ChainPoint *__restrict__ points,
                                                            const uint32_t *__restrict__ point_words, const uint32_t *__restrict__ point_offsets,
                                                            uint32_t blocks, uint32_t w, double *__restrict__ smoothed)
{
	#pragma clang fp contract(off)
	const uint32_t kept = point_offsets[blocks - 1u] + point_words[blocks - 1u], p = blockIdx.x * 256u + threadIdx.x;
	if (p >= kept) return;
	const ChainTrack &t = tracks[points[p].track];
	const uint32_t first = t.first, i = p - first, lo = i > w ? i - w : 0u, hi = i + w < t.length ? i + w : t.length - 1u;
	const ChainPoint *run = points + first;
	double sum[3] = {run[lo].position[0], run[lo].position[1], run[lo].position[2]};
	for (uint32_t j = lo + 1u; j <= hi; j++) {
		#pragma unroll
		for (int r = 0; r < 3; r++) sum[r] = sum[r] + run[j].position[r];
	}
	const double n = (double)(hi - lo + 1u);
	#pragma unroll
	for (int r = 0; r < 3; r++) smoothed[3ull * p + r] = sum[r] / n;
}

/* src, stride: point slot p's three doubles lie at src[p * stride] -- the smoothed list (3), or the positions inside the point records (5) */
__global__ __launch_bounds__(256) void tracks_draw_kernel(const double *__restrict__ src, uint32_t stride, const uint32_t *__restrict__ firsts,
                                                          const uint32_t *__restrict__ stored, const uint2 *__restrict__ links,
                                                          const uint32_t *__restrict__ lengths, const uint32_t *__restrict__ track_of,
                                                          const uint32_t *__restrict__ first_of, const uint32_t *__restrict__ point_offsets,
                                                          BfDrawArgs t, uint32_t *__restrict__ point_map, uint32_t *__restrict__ map_counts,
                                                          unsigned long long *__restrict__ map_sums, BfDrawTally *__restrict__ tallies)
{
	#pragma clang fp contract(off)
	const uint32_t frame = blockIdx.y, n = stored[frame], k = blockIdx.x * 256u + threadIdx.x;
	if (blockIdx.x * 256u >= n) return;
	uint32_t counted[8] = {0, 0, 0, 0, 0, 0, 0, 0};                      /* (BfDrawTally's counters, in its order) */
	if (k < n) {
		const uint32_t i = firsts[frame] + k;
		const uint2 me = links[i];
		const uint32_t h = me.x;
		if (h != BF_TRACK_NONE && track_of[h] != BF_TRACK_NONE) {
			const uint32_t length = lengths[h], slot = point_offsets[h >> 8] + first_of[h] + me.y;
			if (length == 1u) counted[0] = 1u;
			if (me.y + 1u < length) {
				double a[3], d[3], before[3] = {0.0, 0.0, 0.0};
				uint32_t S;
				if (!draw_link(src, stride, slot, a, d, S)) counted[1] = 1u;
				else {
					counted[2] = S;
					/* the sample before the first: the last one of link i - 1, by that link's own numbers; a skipped link is no predecessor */
					bool follows = false;
					if (me.y) {
						double pa[3], pd[3];
						uint32_t pS;
						if (draw_link(src, stride, slot - 1u, pa, pd, pS)) { draw_bin(pa, pd, pS, pS - 1u, before); follows = true; }
					}
					/* the pair call's fixed point, of the smoothed link; |d_r| <= 4096: q_r fits easily */
					const long long q[3] = {(long long)__builtin_floor(d[0] * BF_TRACK_FIXED + 0.5), (long long)__builtin_floor(d[1] * BF_TRACK_FIXED + 0.5),
					                        (long long)__builtin_floor(d[2] * BF_TRACK_FIXED + 0.5)};
					const uint64_t voxels = (uint64_t)t.track_map[0] * t.track_map[1] * t.track_map[2];
					for (uint32_t s = 0; s < S; s++) {
						double B[3];
						draw_bin(a, d, S, s, B);
						const bool repeat = follows && B[0] == before[0] && B[1] == before[1] && B[2] == before[2];
						before[0] = B[0]; before[1] = B[1]; before[2] = B[2];
						follows = true;
						if (repeat) { counted[3]++; continue; }
						if (t.deposit & BF_CHAIN_POINTS) {
							const bool in = B[0] >= 0.0 && B[0] < (double)t.point_map[0] && B[1] >= 0.0 && B[1] < (double)t.point_map[1] &&
							                B[2] >= 0.0 && B[2] < (double)t.point_map[2];
							if (in) atomicAdd(point_map + (((uint64_t)(uint32_t)B[2] * t.point_map[1] + (uint32_t)B[1]) * t.point_map[0] + (uint32_t)B[0]), 1u);
							if (in) counted[4]++; else counted[5]++;
						}
						if (t.deposit & BF_CHAIN_LINKS) {
							const bool in = B[0] >= 0.0 && B[0] < (double)t.track_map[0] && B[1] >= 0.0 && B[1] < (double)t.track_map[1] &&
							                B[2] >= 0.0 && B[2] < (double)t.track_map[2];
							if (in) {
								const uint64_t at = ((uint64_t)(uint32_t)B[2] * t.track_map[1] + (uint32_t)B[1]) * t.track_map[0] + (uint32_t)B[0];
								atomicAdd(map_counts + at, 1u);
								#pragma unroll
								for (int r = 0; r < 3; r++) atomicAdd(map_sums + r * voxels + at, (unsigned long long)q[r]);
							}
							if (in) counted[6]++; else counted[7]++;
						}
					}
				}
			}
		}
	}
	uint32_t *tally = (uint32_t *)(tallies + frame);
	#pragma unroll
	for (int c = 0; c < 8; c++) {
		const uint32_t all = wave_sum(counted[c]);
		if ((threadIdx.x & 63u) == 0 && all) atomicAdd(tally + c, all);
	}
}

namespace {

bool grid_fits(uint32_t frames, uint32_t max_stored)
{
	return frames >= 2 && frames <= 65535u && max_stored >= 1 && max_stored <= BF_TRACK_MAX_PEAKS;
}

/* the chain's pointer-jumping rounds; the links table it leaves is the first half of `links` after an even number, the second after an odd one */
uint32_t jump_rounds(uint32_t frames)
{
	uint32_t rounds = 0;
	while ((1u << rounds) < frames) rounds++;                            /* frames >= 2: at least one, which is also the tails' */
	return rounds;
}

} // namespace

/* list: the emit pass's records, frame n's stored[n] at firsts[n]; placements: frames x 12 doubles; positions: three doubles a record;
 * unplaced[frames]: zeroed by the caller.  All device memory; max_stored: the most records of one frame (host). */
extern "C" hipError_t bf_launch_tracks_place(const void *list, const double *placements, const uint32_t *firsts, const uint32_t *stored,
                                             uint32_t frames, uint32_t max_stored, uint32_t use_offsets, double *positions, uint32_t *unplaced,
                                             hipStream_t s)
{
	if (!list || ((uintptr_t)list & 15u) || !placements || !firsts || !stored || !positions || !unplaced || !grid_fits(frames, max_stored))
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(tracks_place_kernel, dim3((max_stored + 255u) / 256u, frames), dim3(256), 0, s, (const uint4 *)list, placements, firsts, stored,
	                   use_offsets, positions, unplaced);
	return hipGetLastError();
}

/* forward, backward: a uint32 a record, at the record's own index: forward[firsts[n] + a] = f(a) of frame pair n, backward[firsts[n + 1]
 * + b] = g(b) of frame pair n (BF_TRACK_NONE: none).  The oldest frame's backward and the newest frame's forward entries stay unwritten
 * and unread. */
extern "C" hipError_t bf_launch_tracks_nearest(const double *positions, const uint32_t *firsts, const uint32_t *stored, uint32_t frames,
                                               uint32_t max_stored, double r2, uint32_t *forward, uint32_t *backward, hipStream_t s)
{
	if (!positions || !firsts || !stored || !forward || !backward || !grid_fits(frames, max_stored) || !(r2 >= 0.0)) return hipErrorInvalidValue;
	hipLaunchKernelGGL(tracks_nearest_kernel, dim3((max_stored + 255u) / 256u, frames - 1u, 2), dim3(256), 0, s, positions, firsts, stored, r2,
	                   forward, backward);
	return hipGetLastError();
}

/* Three launches: match, scan, emit.  block_firsts[frames - 1]: frame pair n's first block, the pairs before it holding
 * ceil(stored / 256) each, `blocks` in all (host); masks: four words a block; words, offsets: one a block; tallies[frames - 1]: zeroed
 * by the caller.  pairs: NULL, or room for the sum over n of min(stored[n], stored[n + 1]) 48-byte records, 16-byte aligned.  With
 * t->deposit: map_counts, t->points voxels of uint32, and map_sums, three times as many int64 behind one another. */
extern "C" hipError_t bf_launch_tracks_pair(const double *positions, const uint32_t *firsts, const uint32_t *stored, const uint32_t *block_firsts,
                                            uint32_t frames, uint32_t max_stored, uint32_t blocks, const uint32_t *forward, const uint32_t *backward,
                                            uint64_t *masks, uint32_t *words, uint32_t *offsets, const BfTrackArgs *t, uint32_t *map_counts,
                                            void *map_sums, void *pairs, BfTrackTally *tallies, hipStream_t s)
{
	if (!positions || !firsts || !stored || !block_firsts || !forward || !backward || !masks || !words || !offsets || !t || !tallies ||
	    ((uintptr_t)pairs & 15u) || !grid_fits(frames, max_stored) || blocks == 0) return hipErrorInvalidValue;
	if (t->deposit && (!map_counts || !map_sums || !t->points[0] || !t->points[1] || !t->points[2] ||
	                   (uint64_t)t->points[0] * t->points[1] > BF_TRACK_MAX_VOXELS ||
	                   (uint64_t)t->points[0] * t->points[1] * t->points[2] > BF_TRACK_MAX_VOXELS)) return hipErrorInvalidValue;
	const dim3 grid((max_stored + 255u) / 256u, frames - 1u);
	hipLaunchKernelGGL(tracks_match_kernel, grid, dim3(256), 0, s, firsts, stored, block_firsts, forward, backward, masks, words, tallies);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(tracks_scan_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)words, blocks, offsets);
	e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(tracks_emit_kernel, grid, dim3(256), 0, s, positions, firsts, stored, block_firsts, forward, (const uint64_t *)masks,
	                   (const uint32_t *)words, (const uint32_t *)offsets, *t, map_counts, (unsigned long long *)map_sums, (uint4 *)pairs, tallies);
	return hipGetLastError();
}

/* counts: `voxels` uint32; sums: 3 x `voxels` int64; out: `voxels` floats (a frame of the ring); all device memory */
extern "C" hipError_t bf_launch_track_convert(const uint32_t *counts, const void *sums, float *out, uint64_t voxels, uint32_t component,
                                              uint32_t min_pairs, float scale, hipStream_t s)
{
	if (!counts || !sums || !out || voxels == 0 || voxels > BF_TRACK_MAX_VOXELS || component >= BF_TRACK_COMPONENTS) return hipErrorInvalidValue;
	const uint64_t blocks = (voxels + 255u) / 256u;
	hipLaunchKernelGGL(tracks_convert_kernel, dim3((uint32_t)(blocks < 4096u ? blocks : 4096u)), dim3(256), 0, s, counts, (const long long *)sums, out,
	                   voxels, component, min_pairs ? min_pairs : 1u, scale);
	return hipGetLastError();
}

/* (bf_kernels.h says what every table is) */
extern "C" hipError_t bf_launch_tracks_chain(const double *positions, const uint32_t *firsts, const uint32_t *stored, uint32_t frames,
                                             uint32_t max_stored, uint32_t total, const uint32_t *forward, const uint32_t *backward, uint32_t *next,
                                             void *links, uint32_t *lengths, uint32_t *tails, uint32_t *track_of, uint32_t *first_of, uint32_t *words,
                                             uint32_t *offsets, const BfChainArgs *a, uint32_t *point_map, uint32_t *track_counts, void *track_sums,
                                             void *tracks, void *points, BfChainTally *tallies, hipStream_t s)
{
	static_assert(sizeof(BfChainTally) == 32, "eight counters");
	if (!positions || !firsts || !stored || !next || !links || ((uintptr_t)links & 7u) || !lengths || !tails || !track_of || !first_of || !words ||
	    !offsets || !a || !tallies || ((uintptr_t)tracks & 7u) || ((uintptr_t)points & 7u) || !grid_fits(frames, max_stored) || total == 0 ||
	    total > (1u << 26) || (forward == nullptr) != (backward == nullptr) || a->min_length == 0 || (a->deposit & ~(BF_CHAIN_POINTS | BF_CHAIN_LINKS)))
		return hipErrorInvalidValue;
	if ((a->deposit & BF_CHAIN_POINTS) && (!point_map || !a->point_map[0] || !a->point_map[1] || !a->point_map[2] ||
	                                       (uint64_t)a->point_map[0] * a->point_map[1] > BF_MAP_MAX_VOXELS ||
	                                       (uint64_t)a->point_map[0] * a->point_map[1] * a->point_map[2] > BF_MAP_MAX_VOXELS)) return hipErrorInvalidValue;
	if ((a->deposit & BF_CHAIN_LINKS) && (!track_counts || !track_sums || !a->track_map[0] || !a->track_map[1] || !a->track_map[2] ||
	                                      (uint64_t)a->track_map[0] * a->track_map[1] > BF_TRACK_MAX_VOXELS ||
	                                      (uint64_t)a->track_map[0] * a->track_map[1] * a->track_map[2] > BF_TRACK_MAX_VOXELS)) return hipErrorInvalidValue;
	const dim3 by_frame((max_stored + 255u) / 256u, frames);
	const uint32_t blocks = (total + 255u) / 256u;
	uint2 *ping = (uint2 *)links, *pong = ping + total;
	hipLaunchKernelGGL(tracks_link_kernel, by_frame, dim3(256), 0, s, positions, firsts, stored, frames, forward, backward, next, ping, lengths);
	hipError_t e = hipGetLastError();
	const uint32_t rounds = jump_rounds(frames);
	for (uint32_t r = 0; r < rounds && e == hipSuccess; r++) {
		hipLaunchKernelGGL(tracks_jump_kernel, dim3(blocks), dim3(256), 0, s, (const uint2 *)ping, pong, total, (const uint32_t *)next,
		                   r + 1u == rounds ? 1u : 0u, lengths, tails);
		e = hipGetLastError();
		uint2 *swap = ping; ping = pong; pong = swap;                    /* ping: what the next launch reads */
	}
	if (e != hipSuccess) return e;
	uint32_t *track_words = words, *point_words = words + blocks, *track_offsets = offsets, *point_offsets = offsets + blocks;
	hipLaunchKernelGGL(tracks_keep_kernel, dim3(blocks), dim3(256), 0, s, (const uint2 *)ping, (const uint32_t *)lengths, total, a->min_length, track_of,
	                   first_of, track_words, point_words);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL(tracks_scan_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)track_words, blocks, track_offsets);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL(tracks_scan_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t *)point_words, blocks, point_offsets);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL(tracks_finish_kernel, by_frame, dim3(256), 0, s, positions, firsts, stored, frames, (const uint2 *)ping, (const uint32_t *)next,
	                   (const uint32_t *)lengths, (const uint32_t *)tails, (const uint32_t *)track_of, (const uint32_t *)first_of,
	                   (const uint32_t *)track_offsets, (const uint32_t *)point_offsets, *a, point_map, track_counts, (unsigned long long *)track_sums,
	                   (ChainTrack *)tracks, (ChainPoint *)points, tallies);
	return hipGetLastError();
}

/* (bf_kernels.h says what every table is) */
extern "C" hipError_t bf_launch_tracks_draw(const uint32_t *firsts, const uint32_t *stored, uint32_t frames, uint32_t max_stored, uint32_t total,
                                            const void *links, const uint32_t *lengths, const uint32_t *track_of, const uint32_t *first_of,
                                            const uint32_t *words, const uint32_t *offsets, const void *tracks, const void *points, double *smoothed,
                                            const BfDrawArgs *a, uint32_t *point_map, uint32_t *track_counts, void *track_sums, BfDrawTally *tallies,
                                            hipStream_t s)
{
	static_assert(sizeof(BfDrawTally) == 32 && sizeof(ChainPoint) == 5 * sizeof(double) && offsetof(ChainPoint, position) == 2 * sizeof(double),
	              "eight counters; a point record is five doubles wide, its position the last three");
	if (!firsts || !stored || !links || ((uintptr_t)links & 7u) || !lengths || !track_of || !first_of || !words || !offsets || !tracks ||
	    ((uintptr_t)tracks & 7u) || !points || ((uintptr_t)points & 7u) || !a || !tallies || !grid_fits(frames, max_stored) || total == 0 ||
	    total > (1u << 26) || a->smooth > BF_DRAW_MAX_SMOOTH || (a->smooth && !smoothed) || (a->deposit & ~(BF_CHAIN_POINTS | BF_CHAIN_LINKS)))
		return hipErrorInvalidValue;
	if ((a->deposit & BF_CHAIN_POINTS) && (!point_map || !a->point_map[0] || !a->point_map[1] || !a->point_map[2] ||
	                                       (uint64_t)a->point_map[0] * a->point_map[1] > BF_MAP_MAX_VOXELS ||
	                                       (uint64_t)a->point_map[0] * a->point_map[1] * a->point_map[2] > BF_MAP_MAX_VOXELS)) return hipErrorInvalidValue;
	if ((a->deposit & BF_CHAIN_LINKS) && (!track_counts || !track_sums || !a->track_map[0] || !a->track_map[1] || !a->track_map[2] ||
	                                      (uint64_t)a->track_map[0] * a->track_map[1] > BF_TRACK_MAX_VOXELS ||
	                                      (uint64_t)a->track_map[0] * a->track_map[1] * a->track_map[2] > BF_TRACK_MAX_VOXELS)) return hipErrorInvalidValue;
	const uint32_t blocks = (total + 255u) / 256u;
	const uint2 *final_links = (const uint2 *)links + (jump_rounds(frames) & 1u ? total : 0u);
	const uint32_t *point_offsets = offsets + blocks;
	const double *src = (const double *)points + 2;
	uint32_t stride = 5;
	if (a->smooth) {
		hipLaunchKernelGGL(tracks_smooth_kernel, dim3(blocks), dim3(256), 0, s, (const ChainTrack *)tracks, (const ChainPoint *)points, words + blocks,
		                   point_offsets, blocks, a->smooth, smoothed);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return e;
		src = smoothed; stride = 3;
	}
	hipLaunchKernelGGL(tracks_draw_kernel, dim3((max_stored + 255u) / 256u, frames), dim3(256), 0, s, src, stride, firsts, stored, final_links, lengths, track_of, first_of, point_offsets, *a, point_map, track_counts,
	                   (unsigned long long *)track_sums, tallies);
	return hipGetLastError();
}
