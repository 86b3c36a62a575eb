/* frame_quantiles.hip -- exact order statistics of several frames of the frame ring (beamformer_hip_quantiles_last_frames: the
 * thresholds of the peak calls, the noise floor, the display range taken from the frames where they lie).
 *
 * DEFINITION (include/ogl_beamformer_hip.h has it for callers; tests/frame_quantiles_ref.py is its numpy restatement).  The decision
 * value q of a voxel is the one beamformer_hip_find_peaks_last_frames decides on: re * re + im * im for a complex frame, every
 * operation rounded to float32 on its own (contraction off), fabsf(v) for a real one -- no square root takes part.  A voxel is finite
 * when q is; one that is not counts in non_finite and in nothing else.  q is never negative and never -0, so the order of the values is
 * the order of their bit patterns as uint32.  With n the finite voxels of the box and q_(0) <= ... <= q_(n-1) their values, a fraction
 * f (a double in [0, 1]) has the rank r = (uint64)floor(f * (double)(n - 1) + 0.5) -- one double multiply, one add, one floor, no
 * fused multiply-add -- and the value q_(r): a voxel's own value, no interpolation.  below = #{q < value}, equal = #{q == value}, so
 * below <= r < below + equal.  n == 0: all zero.  The coarse histogram: bin b counts the finite voxels with bits >> 20 == b.
 *
 * An MSB-first radix select on the 31 significant bits of q in three digit passes: bits 30..20 (2048 bins), 19..10 and 9..0 (1024 bins
 * each).  A COUNT kernel -- grid y the frame, grid x the block, the box walk of frame_metrics.hip: a thread starts at block * 256 +
 * thread and steps blocks * 256 voxels, the step a host-made (x, y, z) triple, so no division in the loop -- keeps its tables in LDS,
 * adds there with LDS integer atomics, then adds its non-zero bins to the frame's tables in global memory with integer atomics.  Pass 1
 * counts every finite voxel (its table is the coarse histogram, handed out as it is) and non_finite beside it; passes 2 and 3 count a
 * voxel only when its leading bits equal a prefix one of the frame's ranks selected: ranks that share a prefix share a table, at most 16
 * tables of 1024 words a block (4 KiB of LDS a fraction of the call, 64 KiB at the most).  Most voxels match no prefix: a 64-bit mask of the selected prefixes' low six bits, held
 * in scalar registers, turns them away before any compare.  A PICK kernel, one block a frame, follows each count: per rank it scans the
 * rank's table, finds the bin that holds the rank, the count below it and the rank inside it, and writes the frame's distinct prefixes
 * for the next pass; after pass 1 it first forms n and the ranks from the fractions, in double without contraction; after pass 3 the
 * bin is one key: value's bits, below and equal are complete.
 * Integer additions commute: every table and every result repeats byte for byte whatever order the blocks arrive in (the localisation
 * map's argument).  No floating-point atomic exists here.  Bounds: the frames are read three times. */
#include <hip/hip_runtime.h>
#include "bf_kernels.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

/* the bit pattern of the decision value of voxel i */
__device__ __forceinline__ uint32_t decision_bits_at(const float *frame, uint64_t i, uint32_t cplx)
{
	#pragma clang fp contract(off)
	float q;
	if (cplx) { const f32x2 c = ((const f32x2 *)frame)[i]; q = c.x * c.x + c.y * c.y; }
	else q = __builtin_fabsf(frame[i]);
	return __float_as_uint(q);
}

/* finite and so not negative: below 0x7F800000 (a NaN may carry the sign bit) */
__device__ __forceinline__ bool is_finite_bits(uint32_t bits) { return (bits & 0x7F800000u) != 0x7F800000u; }

/* visit(bits) for this thread's voxels of the row's box */
template <class Visit> __device__ __forceinline__ void walk_box(const char *ring, const BfQuantilesRow &row, Visit visit)
{
	const float *frame = (const float *)(ring + row.offset);
	const uint32_t cplx = row.cplx;
	const uint64_t cx = row.count[0], cy = row.count[1], cz = row.count[2];
	const uint64_t px = row.points[0], plane = px * row.points[1];
	/* the start is below blocks * 256 <= 2^18 and the box's extents are 32-bit: 32-bit divisions */
	const uint32_t start = blockIdx.x * 256u + threadIdx.x, rest = start / row.count[0];
	uint64_t x = start - rest * row.count[0], y = rest % row.count[1], z = rest / row.count[1];
	if (rest >= cy * cz) z = cz;                      /* (the last block of a box that is no multiple of 256 voxels: nothing to walk) */
	for (; z < cz;) {
		visit(decision_bits_at(frame, (z + row.first[2]) * plane + (y + row.first[1]) * px + (x + row.first[0]), cplx));
		/* blocks * 256 voxels on: step[0] < cx, step[1] < cy, so one carry an axis */
		x += row.step[0]; if (x >= cx) { x -= cx; y++; }
		y += row.step[1]; if (y >= cy) { y -= cy; z++; }
		z += row.step[2];
	}
}

} // namespace

/* pass 1: table[frame][bits >> 20] over the finite voxels, bad[frame] the others */
__global__ __launch_bounds__(256) void frame_quantiles_count_first_kernel(const char *__restrict__ ring, const BfQuantilesRow *__restrict__ rows,
                                                                          uint32_t *__restrict__ bad, uint32_t *__restrict__ table)
{
	#pragma clang fp contract(off)
	const BfQuantilesRow &row = rows[blockIdx.y];
	if (blockIdx.x >= row.blocks) return;
	__shared__ uint32_t bins[BF_QUANTILES_BINS1];
	__shared__ uint32_t bad_block;
	for (uint32_t b = threadIdx.x; b < BF_QUANTILES_BINS1; b += 256u) bins[b] = 0;
	if (threadIdx.x == 0) bad_block = 0;
	__syncthreads();

	uint32_t mine = 0;
	walk_box(ring, row, [&](uint32_t bits) {
		if (is_finite_bits(bits)) atomicAdd(&bins[bits >> 20], 1u);      /* (finite: the index is below 2040) */
		else mine++;
	});
	if (mine) atomicAdd(&bad_block, mine);
	__syncthreads();

	uint32_t *out = table + (size_t)blockIdx.y * BF_QUANTILES_BINS1;
	for (uint32_t b = threadIdx.x; b < BF_QUANTILES_BINS1; b += 256u) {
		const uint32_t c = bins[b];
		if (c) atomicAdd(&out[b], c);
	}
	if (threadIdx.x == 0 && bad_block) atomicAdd(&bad[blockIdx.y], bad_block);
}

/* passes 2 (SHIFT 20) and 3 (SHIFT 10): table[frame][slot][the ten bits under SHIFT] over the voxels whose bits >> SHIFT are the
 * frame's prefix number `slot`.  A voxel that is not finite has a key from 2040 << (SHIFT - 20) up, which no prefix is.  The LDS is
 * dynamic, 4 KiB a fraction of the call: with the 64 KiB of sixteen tables two blocks fit a CU and the pass took 3.3 times the first
 * one's time on 64 frames of four fractions (measured); a call of few fractions keeps the CU full. */
template <uint32_t SHIFT>
__global__ __launch_bounds__(256) void frame_quantiles_count_next_kernel(const char *__restrict__ ring, const BfQuantilesRow *__restrict__ rows,
                                                                         const BfQuantilesPrefixes *__restrict__ prefixes, uint32_t fraction_count,
                                                                         uint32_t *__restrict__ table)
{
	#pragma clang fp contract(off)
	const BfQuantilesRow &row = rows[blockIdx.y];
	const BfQuantilesPrefixes &selected = prefixes[blockIdx.y];
	const uint32_t tables = selected.tables < fraction_count ? selected.tables : fraction_count;     /* (at most 16: the launch checks) */
	if (blockIdx.x >= row.blocks || tables == 0) return;
	extern __shared__ uint32_t bins[];                           /* fraction_count tables of 1024 words: the launch sizes it */
	for (uint32_t b = threadIdx.x; b < tables * BF_QUANTILES_BINS; b += 256u) bins[b] = 0;
	const uint64_t mask = selected.mask;
	uint32_t prefix[BF_QUANTILES_MAX];
	#pragma unroll
	for (uint32_t t = 0; t < BF_QUANTILES_MAX; t++) prefix[t] = selected.prefix[t];
	__syncthreads();

	walk_box(ring, row, [&](uint32_t bits) {
		const uint32_t key = bits >> SHIFT;
		if (!((mask >> (key & 63u)) & 1u)) return;
		uint32_t slot = BF_QUANTILES_MAX;
		#pragma unroll
		for (uint32_t t = 0; t < BF_QUANTILES_MAX; t++) if (key == prefix[t]) slot = t;
		if (slot < tables) atomicAdd(&bins[slot * BF_QUANTILES_BINS + ((bits >> (SHIFT - 10u)) & (BF_QUANTILES_BINS - 1u))], 1u);
	});
	__syncthreads();

	uint32_t *out = table + (size_t)blockIdx.y * fraction_count * BF_QUANTILES_BINS;
	for (uint32_t b = threadIdx.x; b < tables * BF_QUANTILES_BINS; b += 256u) {
		const uint32_t c = bins[b];
		if (c) atomicAdd(&out[b], c);
	}
}

/* The pick behind count pass `pass` (1, 2, 3), one block a frame, a WAVE a rank (wave w takes ranks w, w + 4, ...): a lane holds
 * `per` consecutive bins of the rank's table (32 of 2048, 16 of 1024), the wave's exclusive scan gives each lane its count below, and
 * the one lane whose bins hold the rank writes the rank's state -- shuffles only, no barrier inside the loop.  Then thread 0 numbers
 * the frame's distinct prefixes.  Counts and ranks are below 2^32 (the box's voxels are). */
__global__ __launch_bounds__(256) void frame_quantiles_pick_kernel(const double *__restrict__ fractions, uint32_t fraction_count, uint32_t pass,
                                                                   const uint32_t *__restrict__ bad, const uint32_t *__restrict__ table,
                                                                   BfQuantilesPrefixes *__restrict__ prefixes, BfQuantilesTally *__restrict__ tallies,
                                                                   BfQuantileState *__restrict__ states)
{
	#pragma clang fp contract(off)
	const uint32_t frame = blockIdx.x, lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t per = pass == 1u ? BF_QUANTILES_BINS1 / 64u : BF_QUANTILES_BINS / 64u;
	__shared__ BfQuantileState chosen[BF_QUANTILES_MAX];
	__shared__ uint32_t voxels;                                  /* n: the sum of the first table */
	__shared__ BfQuantilesPrefixes picked;                       /* (in LDS: thread 0 indexes it with what it finds) */
	const uint32_t n_before = pass == 1u ? 0u : (uint32_t)tallies[frame].voxels;
	if (threadIdx.x == 0 && pass != 1u) voxels = n_before;

	for (uint32_t k = wave; k < fraction_count; k += 4u) {
		BfQuantileState st{};
		if (pass != 1u) st = states[(size_t)frame * fraction_count + k];
		if (pass != 1u && n_before == 0u) {                      /* no finite voxel: no table was counted */
			if (lane == 0) chosen[k] = BfQuantileState{};
			continue;
		}
		const uint32_t *t = pass == 1u ? table + (size_t)frame * BF_QUANTILES_BINS1
		                               : table + ((size_t)frame * fraction_count + (st.slot < fraction_count ? st.slot : 0u)) * BF_QUANTILES_BINS;
		uint32_t c[32], sum = 0;
		#pragma unroll
		for (uint32_t j = 0; j < 32u; j++) { c[j] = j < per ? t[lane * per + j] : 0u; sum += c[j]; }
		uint32_t scan = sum;                                     /* inclusive over the wave */
		for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(scan, off, 64); if ((int)lane >= off) scan += o; }
		const uint32_t total = __shfl(scan, 63, 64);

		uint32_t r;
		if (pass == 1u) {
			if (k == 0 && lane == 0) voxels = total;                 /* (wave 0: there is a rank 0) */
			if (total == 0u) { if (lane == 0) chosen[k] = BfQuantileState{}; continue; }
			const double at = fractions[k] * (double)(total - 1u);
			const double rounded = __builtin_floor(at + 0.5);
			r = (uint32_t)(uint64_t)rounded;
			if (r > total - 1u) r = total - 1u;                  /* (f <= 1: not reached) */
			st.rank = r;
		} else {
			r = st.residual;
		}
		uint32_t cum = scan - sum;
		#pragma unroll
		for (uint32_t j = 0; j < 32u; j++) {
			if (j < per && r >= cum && r - cum < c[j]) {
				const uint32_t bin = lane * per + j;
				st.below += cum;
				st.residual = r - cum;
				st.prefix = pass == 1u ? bin : (st.prefix << 10) | bin;
				st.slot = 0;
				if (pass == 3u) { st.equal = c[j]; st.value_bits = st.prefix; }
				chosen[k] = st;
			}
			cum += c[j];
		}
	}
	__syncthreads();

	if (threadIdx.x == 0) {
		if (pass == 1u) {
			BfQuantilesTally tally;
			tally.voxels = voxels; tally.non_finite = bad[frame];
			tallies[frame] = tally;
		}
		BfQuantilesPrefixes &p = picked;
		p.mask = 0; p.tables = 0; p.reserved = 0;
		for (uint32_t t = 0; t < BF_QUANTILES_MAX; t++) p.prefix[t] = 0xFFFFFFFFu;
		if (pass != 3u && voxels != 0u) {
			for (uint32_t k = 0; k < fraction_count; k++) {
				uint32_t slot = 0;
				while (slot < p.tables && p.prefix[slot] != chosen[k].prefix) slot++;
				if (slot == p.tables) { p.prefix[slot] = chosen[k].prefix; p.tables++; p.mask |= 1ull << (chosen[k].prefix & 63u); }
				chosen[k].slot = slot;
			}
		}
		if (pass != 3u) prefixes[frame] = p;
	}
	__syncthreads();
	if (threadIdx.x < fraction_count) states[(size_t)frame * fraction_count + threadIdx.x] = chosen[threadIdx.x];
}

extern "C" hipError_t bf_launch_frame_quantiles(const void *ring, const BfQuantilesRow *rows, const double *fractions, uint32_t frame_count,
                                                uint32_t fraction_count, uint32_t max_blocks, uint32_t *tables, BfQuantilesPrefixes *prefixes,
                                                BfQuantilesTally *tallies, BfQuantileState *states, hipStream_t s)
{
	if (!ring || !rows || !fractions || !tables || !prefixes || !tallies || !states || frame_count == 0 || frame_count > 65535u ||
	    fraction_count == 0 || fraction_count > BF_QUANTILES_MAX || max_blocks == 0 || max_blocks > BF_METRICS_MAX_BLOCKS)
		return hipErrorInvalidValue;
	hipError_t e = hipMemsetAsync(tables, 0, sizeof(uint32_t) * bf_quantiles_table_words(frame_count, fraction_count), s);
	if (e != hipSuccess) return e;
	uint32_t *bad = tables, *first = tables + bf_quantiles_pass1_at(frame_count);
	uint32_t *second = first + (size_t)frame_count * BF_QUANTILES_BINS1, *third = second + bf_quantiles_pass_words(frame_count, fraction_count);
	const dim3 grid(max_blocks, frame_count);
	const uint32_t lds = fraction_count * BF_QUANTILES_BINS * (uint32_t)sizeof(uint32_t);      /* at most 64 KiB */
	hipLaunchKernelGGL(frame_quantiles_count_first_kernel, grid, dim3(256), 0, s, (const char *)ring, rows, bad, first);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL(frame_quantiles_pick_kernel, dim3(frame_count), dim3(256), 0, s, fractions, fraction_count, 1u, bad, first, prefixes, tallies, states);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL(frame_quantiles_count_next_kernel<20u>, grid, dim3(256), lds, s, (const char *)ring, rows, prefixes, fraction_count, second);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL(frame_quantiles_pick_kernel, dim3(frame_count), dim3(256), 0, s, fractions, fraction_count, 2u, bad, second, prefixes, tallies, states);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL(frame_quantiles_count_next_kernel<10u>, grid, dim3(256), lds, s, (const char *)ring, rows, prefixes, fraction_count, third);
	if ((e = hipGetLastError()) != hipSuccess) return e;
	hipLaunchKernelGGL(frame_quantiles_pick_kernel, dim3(frame_count), dim3(256), 0, s, fractions, fraction_count, 3u, bad, third, prefixes, tallies, states);
	return hipGetLastError();
}
