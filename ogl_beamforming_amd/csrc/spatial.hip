/* spatial.hip -- the separable spatial filter on the frames of the frame ring (beamformer_hip_convolve_last_frames): one launch a live
 * axis, the passes in the order x, y, z, each reading the float32 field the one before it stored.  include/ogl_beamformer_hip.h has
 * the definition for callers; tests/spatial_ref.py restates it in numpy.
 *
 * A PASS along an axis of `extent` points with n = 2r + 1 taps h: out[i] = the float32 fmaf chain from +0 in ascending t of
 * fmaf(h[t], in[i + r - t], acc), the terms whose source index lies outside 0 .. extent - 1 skipped.  A complex voxel is two such
 * chains under the same real taps.  The host describes every axis the same way -- `inner` contiguous voxels, then `extent` points at
 * a stride of `inner`, then `outer` slices at a stride of inner * extent (x: 1, nx, ny nz; y: nx, ny, nz; z: nx ny, nz, 1) -- and two
 * kernels cover the cases.
 *
 * spatial_row_kernel (inner == 1: the axis is the contiguous one).  A block of 256 lanes owns 256 / P rows (16 at the most) of P
 * voxels each, P the power of two that holds min(extent, 256): a lane one output voxel.  The rows' segments and their halos of r voxels
 * either side are staged in LDS with coalesced 8-byte loads (4-byte for real frames), then every lane walks the taps over LDS:
 * one ds_read and the fma per tap, the tap a scalar operand (a scalar load from the call's device table, the index uniform).  A
 * source voxel crosses HBM once; the halo, 2r of P + 2r voxels, comes from L2.  LDS: 768 voxels (6 KiB), 3 KiB more in the
 * Normalised passes that read D.
 *
 * spatial_run_kernel (inner > 1: lanes lie across the contiguous voxels, the axis runs at a stride).  A lane owns one of the `inner`
 * positions and kRun = 16 consecutive outputs along the axis: 16 chains in registers.  It walks the kRun + 2r source points of its run
 * once, from the far end down -- descending source index is ascending tap index for every chain --, four loads in flight ahead of
 * their fma, and each loaded voxel feeds the chains whose support covers it.  Which chains those are, and which tap, depends on the
 * point's index alone: uniform across the wave, so the tap is a scalar operand and the choice a scalar branch; a group's taps are one
 * window of the table, loaded as one batch.  A source voxel is
 * loaded (kRun + 2r) / kRun times, 1.5 at 9 taps, the excess from L2 / Infinity Cache; every load and store is a whole coalesced row
 * segment.  No LDS.  A block is one wave: a view plane of 512 x 1024 still gives 512 blocks.
 *
 * NORMALISED MODE carries the denominator field D, one float a voxel, beside the numerator: STAGE 1 (the first pass) reads the source
 * frame, takes m = 1 where both floats of a voxel are finite and skips the terms of the others; STAGE 2 (a later pass) reads D as the
 * pass before stored it.  The last pass stores N / D (IEEE division) and no D.  STAGE 0 is Zero mode: plain IEEE, nothing skipped
 * but what lies outside the frame.
 *
 * No atomics, no scratch memory; __launch_bounds__ are the launch's block sizes. */
#include <hip/hip_runtime.h>
#include "bf_kernels.h"

typedef float spatial_f32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr uint32_t kRowBlock = 256u;                      /* lanes, and output voxels, of a block of spatial_row_kernel */
constexpr uint32_t kRowRows  = 16u;                       /* rows a block stages at the most */
constexpr uint32_t kRowLds   = kRowRows * (kRowBlock / kRowRows + 2u * (BF_SPATIAL_MAX_TAPS / 2u));   /* 16 x (16 + 32): the largest rows x (P + 2r) */
constexpr uint32_t kRun      = 16u;                       /* outputs along the axis a lane of spatial_run_kernel owns */
constexpr uint32_t kAhead    = 4u;                        /* source points loaded ahead of their fma */
constexpr uint32_t kRunBlock = 64u;

static_assert(BF_SPATIAL_MAX_TAPS % 2u == 1u, "a centre tap");
static_assert(kRun - 1u <= BF_SPATIAL_TAP_FRONT && BF_SPATIAL_TAP_FRONT + (BF_SPATIAL_MAX_TAPS - 1u) + kRun + kAhead - 1u <= BF_SPATIAL_TAP_STRIDE,
              "the window of taps a group of spatial_run_kernel reads lies inside the axis's row of the table");
static_assert(kRowLds >= kRowBlock + 2u * (BF_SPATIAL_MAX_TAPS / 2u), "one row of 256 voxels and its halo");

template <bool CPLX> struct Voxel;
template <> struct Voxel<true>  { typedef spatial_f32x2 type; };
template <> struct Voxel<false> { typedef float type; };

__device__ __forceinline__ bool finite_of(float v)         { return __builtin_isfinite(v); }
__device__ __forceinline__ bool finite_of(spatial_f32x2 v) { return __builtin_isfinite(v.x) && __builtin_isfinite(v.y); }
__device__ __forceinline__ float zero_of(float)            { return 0.0f; }
__device__ __forceinline__ spatial_f32x2 zero_of(spatial_f32x2) { spatial_f32x2 z; z.x = 0.0f; z.y = 0.0f; return z; }
__device__ __forceinline__ float term(float h, float v, float acc) { return __builtin_fmaf(h, v, acc); }
__device__ __forceinline__ spatial_f32x2 term(float h, spatial_f32x2 v, spatial_f32x2 acc)
{
	acc.x = __builtin_fmaf(h, v.x, acc.x); acc.y = __builtin_fmaf(h, v.y, acc.y);
	return acc;
}
__device__ __forceinline__ float quotient(float n, float d) { return n / d; }
__device__ __forceinline__ spatial_f32x2 quotient(spatial_f32x2 n, float d) { n.x = n.x / d; n.y = n.y / d; return n; }

__device__ __forceinline__ float real_of(float v)          { return v; }
__device__ __forceinline__ float real_of(spatial_f32x2 v)  { return v.x; }
__device__ __forceinline__ float imag_of(float)            { return 0.0f; }
__device__ __forceinline__ float imag_of(spatial_f32x2 v)  { return v.y; }
template <class T> __device__ __forceinline__ T voxel_of(float re, float im);
template <> __device__ __forceinline__ float voxel_of<float>(float re, float) { return re; }
template <> __device__ __forceinline__ spatial_f32x2 voxel_of<spatial_f32x2>(float re, float im) { spatial_f32x2 v; v.x = re; v.y = im; return v; }

/* frame k of the pass's input: a ring frame at its own offset (the first pass), or frame k of a contiguous run */
__device__ __forceinline__ const char *frame_in(const char *in, const uint64_t *offsets, const BfSpatialArgs &a, uint32_t k)
{
	return in + (offsets ? offsets[k] : (uint64_t)k * a.in_stride);
}

} // namespace

template <bool CPLX, uint32_t STAGE>
__global__ __launch_bounds__(kRowBlock) void spatial_row_kernel(const char *__restrict__ in, const uint64_t *__restrict__ offsets, char *__restrict__ out,
                                                                const float *__restrict__ d_in, float *__restrict__ d_out,
                                                                const float *__restrict__ taps, BfSpatialArgs a)
{
	typedef typename Voxel<CPLX>::type T;
	__shared__ T tile[kRowLds];
	__shared__ float dtile[STAGE == 2u ? kRowLds : 1u];

	const uint32_t r = a.taps / 2u, P = 1u << a.row_log2, rows = a.row_rows, pitch = P + 2u * r;
	uint32_t b = blockIdx.x;
	const uint32_t seg = b % a.row_segments; b /= a.row_segments;
	const uint32_t group = b % a.row_groups, k = b / a.row_groups;
	const uint32_t row0 = group * rows, x0 = seg * P;
	const T *src = (const T *)frame_in(in, offsets, a, k);
	const float *dsrc = STAGE == 2u ? d_in + (uint64_t)k * a.d_stride : nullptr;

	for (uint32_t j = 0; j < rows && row0 + j < a.outer; j++) {
		const uint64_t base = (uint64_t)(row0 + j) * a.extent;
		for (uint32_t q = threadIdx.x; q < pitch; q += kRowBlock) {
			const int64_t x = (int64_t)x0 + q - r;
			if (x >= 0 && x < (int64_t)a.extent) {
				tile[j * pitch + q] = src[base + (uint64_t)x];
				if (STAGE == 2u) dtile[j * pitch + q] = dsrc[base + (uint64_t)x];
			}
		}
	}
	__syncthreads();

	const uint32_t j = threadIdx.x >> a.row_log2, xl = threadIdx.x & (P - 1u), x = x0 + xl;
	if (j >= rows || row0 + j >= a.outer || x >= a.extent) return;
	T acc = zero_of(T());
	float den = 0.0f;
	const T *line = tile + j * pitch + xl + 2u * r;                /* line[-t]: the source voxel of tap t */
	const float *dline = dtile + (STAGE == 2u ? j * pitch + xl + 2u * r : 0u);
	/* unrolled to the limit: the index of every tap is a constant, so the scalar loads of the taps are issued together, ahead of the loop */
	#pragma unroll
	for (uint32_t t = 0; t < BF_SPATIAL_MAX_TAPS; t++) {
		if (t >= a.taps) break;
		const int64_t xs = (int64_t)x + r - t;
		if (xs < 0 || xs >= (int64_t)a.extent) continue;
		const float h = taps[t];
		const T v = line[-(int32_t)t];
		if (STAGE == 1u) {
			if (finite_of(v)) { acc = term(h, v, acc); den = __builtin_fmaf(h, 1.0f, den); }
		} else {
			acc = term(h, v, acc);
			if (STAGE == 2u) den = __builtin_fmaf(h, dline[-(int32_t)t], den);
		}
	}
	const uint64_t e = (uint64_t)(row0 + j) * a.extent + x;
	T *dst = (T *)(out + (uint64_t)k * a.out_stride);
	if (STAGE != 0u && a.last) acc = quotient(acc, den);
	dst[e] = acc;
	if (STAGE != 0u && !a.last) d_out[(uint64_t)k * a.d_stride + e] = den;
}

template <bool CPLX, uint32_t STAGE>
__global__ __launch_bounds__(kRunBlock) void spatial_run_kernel(const char *__restrict__ in, const uint64_t *__restrict__ offsets, char *__restrict__ out,
                                                                const float *__restrict__ d_in, float *__restrict__ d_out,
                                                                const float *__restrict__ taps, BfSpatialArgs a)
{
	typedef typename Voxel<CPLX>::type T;
	const uint32_t r = a.taps / 2u;
	uint32_t b = blockIdx.x;
	const uint32_t bi = b % a.run_blocks; b /= a.run_blocks;
	const uint32_t chunk = b % a.run_chunks; b /= a.run_chunks;
	const uint32_t o = b % a.outer, k = b / a.outer;
	const uint32_t q = bi * kRunBlock + threadIdx.x;
	if (q >= a.inner) return;
	const uint64_t column = (uint64_t)o * a.extent * a.inner + q;      /* the lane's voxel at point 0 of the axis */
	const T *src = (const T *)frame_in(in, offsets, a, k) + column;
	const float *dsrc = STAGE == 2u ? d_in + (uint64_t)k * a.d_stride + column : nullptr;

	const uint32_t a0 = chunk * kRun;                                   /* the run's first output point */
	const uint32_t count = a.extent - a0 < kRun ? a.extent - a0 : kRun; /* its outputs */
	/* the source points of the run, clipped to the frame: lo .. hi */
	const uint32_t lo = a0 > r ? a0 - r : 0u;
	const uint32_t hi = a0 + count - 1u + r < a.extent - 1u ? a0 + count - 1u + r : a.extent - 1u;

	float re[kRun], im[kRun], den[kRun];                                /* (im, den: unused where the instantiation has none) */
	#pragma unroll
	for (uint32_t i = 0; i < kRun; i++) { re[i] = 0.0f; im[i] = 0.0f; den[i] = 0.0f; }

	/* groups of kAhead points from hi down: point s = top - u; the points below lo are not loaded and take no part */
	for (int64_t top = hi; top >= (int64_t)lo; top -= kAhead) {
		float vr[kAhead], vi[kAhead], dv[kAhead];
		#pragma unroll
		for (uint32_t u = 0; u < kAhead; u++) {
			const int64_t s = top - u;
			vr[u] = 0.0f; vi[u] = 0.0f; dv[u] = 0.0f;
			if (s >= (int64_t)lo) {
				const T v = src[(uint64_t)s * a.inner];
				vr[u] = real_of(v); vi[u] = imag_of(v);
				if (STAGE == 2u) dv[u] = dsrc[(uint64_t)s * a.inner];
			}
		}
		/* output a0 + i takes source s = top - u under tap t = (a0 + i) + r - s = base + i + u: the group's taps are a window of the
		 * table at constant offsets from `base` -- one batch of scalar loads a group, in flight with the group's vector loads (the
		 * table is readable, and never used, BF_SPATIAL_TAP_FRONT floats in front of the taps and to BF_SPATIAL_TAP_STRIDE behind) */
		const int32_t base = (int32_t)(a0 + r) - (int32_t)top;
		float hw[kRun + kAhead - 1u];
		#pragma unroll
		for (uint32_t j = 0; j < kRun + kAhead - 1u; j++) hw[j] = taps[base + (int32_t)j];
		#pragma unroll
		for (uint32_t u = 0; u < kAhead; u++) {
			const int64_t s = top - u;
			if (s < (int64_t)lo) break;
			const bool keep = STAGE != 1u || (__builtin_isfinite(vr[u]) && __builtin_isfinite(vi[u]));
			#pragma unroll
			for (uint32_t i = 0; i < kRun; i++) {
				const int32_t t = base + (int32_t)(i + u);
				if (t >= 0 && t < (int32_t)a.taps) {
					const float h = hw[i + u];
					if (keep) {
						re[i] = __builtin_fmaf(h, vr[u], re[i]);
						if (CPLX) im[i] = __builtin_fmaf(h, vi[u], im[i]);
						if (STAGE == 1u) den[i] = __builtin_fmaf(h, 1.0f, den[i]);
						if (STAGE == 2u) den[i] = __builtin_fmaf(h, dv[u], den[i]);
					}
				}
			}
		}
	}

	T *dst = (T *)(out + (uint64_t)k * a.out_stride) + column;
	float *ddst = d_out + (STAGE != 0u && !a.last ? (uint64_t)k * a.d_stride + column : 0u);
	#pragma unroll
	for (uint32_t i = 0; i < kRun; i++) {
		if (i < count) {
			const uint64_t at = (uint64_t)(a0 + i) * a.inner;
			const T n = voxel_of<T>(re[i], im[i]);
			dst[at] = STAGE != 0u && a.last ? quotient(n, den[i]) : n;
			if (STAGE != 0u && !a.last) ddst[at] = den[i];
		}
	}
}

namespace {

template <bool CPLX, uint32_t STAGE>
hipError_t launch(const void *in, const uint64_t *offsets, void *out, const float *d_in, float *d_out, const float *taps, const BfSpatialArgs &a,
                  bool row, uint32_t blocks, hipStream_t s)
{
	if (row) hipLaunchKernelGGL((spatial_row_kernel<CPLX, STAGE>), dim3(blocks), dim3(kRowBlock), 0, s, (const char *)in, offsets, (char *)out, d_in, d_out, taps, a);
	else     hipLaunchKernelGGL((spatial_run_kernel<CPLX, STAGE>), dim3(blocks), dim3(kRunBlock), 0, s, (const char *)in, offsets, (char *)out, d_in, d_out, taps, a);
	return hipGetLastError();
}

} // namespace

/* One pass.  Every table and field is device memory; the input frames (offsets: inside `in`; else frame k at in + k * in_stride), the
 * output run and the D fields hold frames * inner * extent * outer voxels each and do not overlap: the caller's business
 * (frame_ops.cpp: convolve_last_frames), nothing here re-checks it.  The launch geometry in `args` is filled in here. */
extern "C" hipError_t bf_launch_spatial(const void *in, const uint64_t *offsets, void *out, const float *d_in, float *d_out, const float *taps,
                                        const BfSpatialArgs *args, hipStream_t s)
{
	if (!in || !out || !taps || !args) return hipErrorInvalidValue;
	BfSpatialArgs a = *args;
	if (a.frames == 0 || a.frames > BF_ENSEMBLE_MAX_FRAMES || a.taps == 0 || a.taps > BF_SPATIAL_MAX_TAPS || a.taps % 2u == 0 || a.stage > 2u ||
	    a.inner == 0 || a.extent == 0 || a.outer == 0)
		return hipErrorInvalidValue;
	if ((a.stage == 2u && !d_in) || (a.stage != 0u && !a.last && !d_out)) return hipErrorInvalidValue;
	uint64_t blocks;
	const bool row = a.inner == 1u;
	if (row) {
		a.row_log2 = 0;
		while ((1u << a.row_log2) < kRowBlock && (1u << a.row_log2) < a.extent) a.row_log2++;
		const uint32_t P = 1u << a.row_log2;
		a.row_rows = kRowBlock / P < kRowRows ? kRowBlock / P : kRowRows;
		a.row_segments = (a.extent + P - 1u) / P;
		a.row_groups = (a.outer + a.row_rows - 1u) / a.row_rows;
		if (a.row_rows * (P + 2u * (a.taps / 2u)) > kRowLds) return hipErrorInvalidValue;
		blocks = (uint64_t)a.row_segments * a.row_groups * a.frames;
	} else {
		a.run_blocks = (a.inner + kRunBlock - 1u) / kRunBlock;
		a.run_chunks = (a.extent + kRun - 1u) / kRun;
		blocks = (uint64_t)a.run_blocks * a.run_chunks * a.outer * a.frames;
	}
	if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
	const uint32_t n = (uint32_t)blocks;
	if (a.cplx) {
		switch (a.stage) {
		case 0:  return launch<true, 0>(in, offsets, out, d_in, d_out, taps, a, row, n, s);
		case 1:  return launch<true, 1>(in, offsets, out, d_in, d_out, taps, a, row, n, s);
		default: return launch<true, 2>(in, offsets, out, d_in, d_out, taps, a, row, n, s);
		}
	}
	switch (a.stage) {
	case 0:  return launch<false, 0>(in, offsets, out, d_in, d_out, taps, a, row, n, s);
	case 1:  return launch<false, 1>(in, offsets, out, d_in, d_out, taps, a, row, n, s);
	default: return launch<false, 2>(in, offsets, out, d_in, d_out, taps, a, row, n, s);
	}
}
