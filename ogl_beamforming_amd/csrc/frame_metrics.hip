/* frame_metrics.hip -- focus metrics of several frames of the frame ring in two launches (beamformer_hip_score_last_frames: the K frames
 * of a variants push scored where they lie, so that a caller keeps the sharpest without downloading any of them).
 *
 * DEFINITION (include/ogl_beamformer_hip.h has it for callers; tests/frame_metrics_ref.py is its numpy restatement).  The magnitude of
 * a voxel is ONE float32: sqrtf(re * re + im * im) for a complex frame, every operation rounded on its own (contraction off, as
 * stages.hip's sum_kernel: the library builds at -O3, which would fuse the multiply and the add), fabsf(v) for a real one.  A voxel is
 * finite when that float is.  Everything else is formed in double from that float: a = (double)|v|, the powers a, a * a and
 * (a * a) * (a * a), the gradient term d = (double)|v[i + 1]| - (double)|v[i]|, then d * d.  A voxel that is not finite counts in
 * `bad` and in nothing else; a pair with such a voxel is no pair; pairs lie inside the box.
 *
 * Partial pass: grid y the frame, grid x the block within it.  A frame's BfMetricsRow says where it lies, its grid and kind, the box
 * and how many blocks walk it -- a function of the box alone (bf_metrics_blocks), so the bits of a frame's result depend on nothing but
 * that frame and the box; blocks past that number leave at once.  A thread walks the box's voxels (x fastest) from block * 256 + thread
 * in steps of blocks * 256; the step arrives from the host as an (x, y, z) triple, so the walk is additions and carries -- no division
 * in the loop, and the one at its start is 32-bit (the start is below 2^18).  Per voxel: the magnitude once, and the +x, +y, +z
 * neighbours' magnitudes where the neighbour is inside the box, by plain loads (the +x one hits the line the voxel came from, the others
 * lines a neighbouring lane or block loads anyway).  Reduction: wave by butterfly, block through LDS in wave order, one BfMetricsPartial
 * a block.  Final pass: one wave a frame folds its partials -- lane l those numbered l, l + 64, ... in that order, then the butterfly.
 * No atomics anywhere: the order of every addition is fixed by the box, so a frame's bits repeat.  The maximum carries its flat index
 * in the frame through every fold under "larger value, else lower index", which is independent of the partition. */
#include <hip/hip_runtime.h>
#include "bf_kernels.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

/* what a thread, a wave, a block holds: the counts in 32 bits (a block walks at most volume / blocks voxels) */
struct Tally {
	double   s1, s2, s4, g0, g1, g2;
	uint64_t max_index;
	float    max_abs;                  /* -1: no finite voxel yet */
	uint32_t n, bad, p0, p1, p2;
};

__device__ __forceinline__ void clear(Tally &t)
{
	t.s1 = t.s2 = t.s4 = t.g0 = t.g1 = t.g2 = 0.0;
	t.max_index = ~0ull; t.max_abs = -1.0f;
	t.n = t.bad = t.p0 = t.p1 = t.p2 = 0;
}

/* a += b.  Symmetric: both lanes of a butterfly step arrive at the same bits. */
__device__ __forceinline__ void fold(Tally &a, const Tally &b)
{
	a.s1 += b.s1; a.s2 += b.s2; a.s4 += b.s4; a.g0 += b.g0; a.g1 += b.g1; a.g2 += b.g2;
	a.n += b.n; a.bad += b.bad; a.p0 += b.p0; a.p1 += b.p1; a.p2 += b.p2;
	if (b.max_abs > a.max_abs || (b.max_abs == a.max_abs && b.max_index < a.max_index)) { a.max_abs = b.max_abs; a.max_index = b.max_index; }
}

__device__ __forceinline__ Tally from_lane_xor(const Tally &t, int off)
{
	Tally o;
	o.s1 = __shfl_xor(t.s1, off, 64); o.s2 = __shfl_xor(t.s2, off, 64); o.s4 = __shfl_xor(t.s4, off, 64);
	o.g0 = __shfl_xor(t.g0, off, 64); o.g1 = __shfl_xor(t.g1, off, 64); o.g2 = __shfl_xor(t.g2, off, 64);
	o.max_index = __shfl_xor((unsigned long long)t.max_index, off, 64); o.max_abs = __shfl_xor(t.max_abs, off, 64);
	o.n = __shfl_xor(t.n, off, 64); o.bad = __shfl_xor(t.bad, off, 64);
	o.p0 = __shfl_xor(t.p0, off, 64); o.p1 = __shfl_xor(t.p1, off, 64); o.p2 = __shfl_xor(t.p2, off, 64);
	return o;
}

__device__ __forceinline__ float magnitude_at(const float *frame, uint64_t i, uint32_t cplx)
{
	#pragma clang fp contract(off)
	if (cplx) { f32x2 c = ((const f32x2 *)frame)[i]; return __builtin_sqrtf(c.x * c.x + c.y * c.y); }
	return __builtin_fabsf(frame[i]);
}

__device__ __forceinline__ bool is_finite(float a) { return (__float_as_uint(a) & 0x7F800000u) != 0x7F800000u; }

/* the pair (a, its neighbour b): one more pair and (b - a)^2, when b is finite too */
__device__ __forceinline__ void pair_term(double a, float b, uint32_t &pairs, double &g)
{
	#pragma clang fp contract(off)
	if (is_finite(b)) { const double d = (double)b - a; pairs++; g = g + d * d; }
}

} // namespace

__global__ __launch_bounds__(256) void frame_metrics_partial_kernel(const char *__restrict__ ring, const BfMetricsRow *__restrict__ rows,
                                                                    BfMetricsPartial *__restrict__ partials)
{
	#pragma clang fp contract(off)
	const BfMetricsRow &row = rows[blockIdx.y];
	if (blockIdx.x >= row.blocks) return;
	const float *frame = (const float *)(ring + row.offset);
	const uint32_t cplx = row.cplx;
	const uint64_t cx = row.count[0], cy = row.count[1], cz = row.count[2];
	const uint64_t px = row.points[0], plane = px * row.points[1];

	Tally t;
	clear(t);
	/* the start is below blocks * 256 <= 2^18 and the box's extents are 32-bit: 32-bit divisions */
	const uint32_t start = blockIdx.x * 256u + threadIdx.x, rest = start / row.count[0];
	uint64_t x = start - rest * row.count[0], y = rest % row.count[1], z = rest / row.count[1];
	if (rest >= cy * cz) z = cz;                      /* (the last block of a box that is no multiple of 256 voxels: nothing to walk) */
	for (; z < cz;) {
		const uint64_t i = (z + row.first[2]) * plane + (y + row.first[1]) * px + (x + row.first[0]);
		const float m = magnitude_at(frame, i, cplx);
		if (is_finite(m)) {
			const double a = (double)m, a2 = a * a;
			t.n++;
			t.s1 = t.s1 + a; t.s2 = t.s2 + a2; t.s4 = t.s4 + a2 * a2;
			if (m > t.max_abs) { t.max_abs = m; t.max_index = i; }          /* (a thread's indices grow: the first maximum stays) */
			if (x + 1 < cx) pair_term(a, magnitude_at(frame, i + 1, cplx), t.p0, t.g0);
			if (y + 1 < cy) pair_term(a, magnitude_at(frame, i + px, cplx), t.p1, t.g1);
			if (z + 1 < cz) pair_term(a, magnitude_at(frame, i + plane, cplx), t.p2, t.g2);
		} else {
			t.bad++;
		}
		/* blocks * 256 voxels on: step[0] < cx, step[1] < cy, so one carry an axis */
		x += row.step[0]; if (x >= cx) { x -= cx; y++; }
		y += row.step[1]; if (y >= cy) { y -= cy; z++; }
		z += row.step[2];
	}

	for (int off = 32; off > 0; off >>= 1) { const Tally o = from_lane_xor(t, off); fold(t, o); }
	__shared__ Tally waves[4];
	if ((threadIdx.x & 63u) == 0) waves[threadIdx.x >> 6] = t;
	__syncthreads();
	if (threadIdx.x == 0) {
		fold(t, waves[1]); fold(t, waves[2]); fold(t, waves[3]);
		BfMetricsPartial p;
		p.s1 = t.s1; p.s2 = t.s2; p.s4 = t.s4; p.g[0] = t.g0; p.g[1] = t.g1; p.g[2] = t.g2;
		p.max_index = t.max_index; p.max_abs = t.max_abs;
		p.n = t.n; p.bad = t.bad; p.pairs[0] = t.p0; p.pairs[1] = t.p1; p.pairs[2] = t.p2;
		partials[row.partial_first + blockIdx.x] = p;
	}
}

namespace {

struct Total {
	double   s1, s2, s4, g0, g1, g2;
	uint64_t max_index, n, bad, p0, p1, p2;
	float    max_abs;
};

__device__ __forceinline__ void fold(Total &a, const Total &b)
{
	a.s1 += b.s1; a.s2 += b.s2; a.s4 += b.s4; a.g0 += b.g0; a.g1 += b.g1; a.g2 += b.g2;
	a.n += b.n; a.bad += b.bad; a.p0 += b.p0; a.p1 += b.p1; a.p2 += b.p2;
	if (b.max_abs > a.max_abs || (b.max_abs == a.max_abs && b.max_index < a.max_index)) { a.max_abs = b.max_abs; a.max_index = b.max_index; }
}

__device__ __forceinline__ uint64_t xor_u64(uint64_t v, int off) { return __shfl_xor((unsigned long long)v, off, 64); }

} // namespace

__global__ __launch_bounds__(64) void frame_metrics_final_kernel(const BfMetricsRow *__restrict__ rows, const BfMetricsPartial *__restrict__ partials,
                                                                 BfMetricsResult *__restrict__ results)
{
	#pragma clang fp contract(off)
	const BfMetricsRow &row = rows[blockIdx.x];
	Total t;
	t.s1 = t.s2 = t.s4 = t.g0 = t.g1 = t.g2 = 0.0;
	t.max_index = ~0ull; t.max_abs = -1.0f;
	t.n = t.bad = t.p0 = t.p1 = t.p2 = 0;
	for (uint32_t k = threadIdx.x; k < row.blocks; k += 64u) {
		const BfMetricsPartial p = partials[row.partial_first + k];
		Total o;
		o.s1 = p.s1; o.s2 = p.s2; o.s4 = p.s4; o.g0 = p.g[0]; o.g1 = p.g[1]; o.g2 = p.g[2];
		o.max_index = p.max_index; o.max_abs = p.max_abs;
		o.n = p.n; o.bad = p.bad; o.p0 = p.pairs[0]; o.p1 = p.pairs[1]; o.p2 = p.pairs[2];
		fold(t, o);
	}
	for (int off = 32; off > 0; off >>= 1) {
		Total o;
		o.s1 = __shfl_xor(t.s1, off, 64); o.s2 = __shfl_xor(t.s2, off, 64); o.s4 = __shfl_xor(t.s4, off, 64);
		o.g0 = __shfl_xor(t.g0, off, 64); o.g1 = __shfl_xor(t.g1, off, 64); o.g2 = __shfl_xor(t.g2, off, 64);
		o.max_index = xor_u64(t.max_index, off); o.max_abs = __shfl_xor(t.max_abs, off, 64);
		o.n = xor_u64(t.n, off); o.bad = xor_u64(t.bad, off);
		o.p0 = xor_u64(t.p0, off); o.p1 = xor_u64(t.p1, off); o.p2 = xor_u64(t.p2, off);
		fold(t, o);
	}
	if (threadIdx.x == 0) {
		BfMetricsResult r;
		r.s1 = t.s1; r.s2 = t.s2; r.s4 = t.s4; r.g[0] = t.g0; r.g[1] = t.g1; r.g[2] = t.g2;
		r.voxels = t.n; r.bad = t.bad; r.pairs[0] = t.p0; r.pairs[1] = t.p1; r.pairs[2] = t.p2;
		r.max_index = t.n ? t.max_index : 0;
		r.max_abs = t.n ? t.max_abs : 0.0f;
		r.reserved = 0;
		results[blockIdx.x] = r;
	}
}

/* rows, partials, results: device memory; rows[k].partial_first + rows[k].blocks partials, frame_count results.  Every row's box lies
 * inside its frame and its frame inside the ring: the caller's business (frame_ops.cpp: score_last_frames), nothing here re-checks it. */
extern "C" hipError_t bf_launch_frame_metrics(const void *ring, const BfMetricsRow *rows, uint32_t frame_count, uint32_t max_blocks,
                                              BfMetricsPartial *partials, BfMetricsResult *results, hipStream_t s)
{
	if (!ring || !rows || !partials || !results || frame_count == 0 || frame_count > 65535u || max_blocks == 0 || max_blocks > BF_METRICS_MAX_BLOCKS)
		return hipErrorInvalidValue;
	hipLaunchKernelGGL(frame_metrics_partial_kernel, dim3(max_blocks, frame_count), dim3(256), 0, s, (const char *)ring, rows, partials);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(frame_metrics_final_kernel, dim3(frame_count), dim3(64), 0, s, rows, partials, results);
	return hipGetLastError();
}
