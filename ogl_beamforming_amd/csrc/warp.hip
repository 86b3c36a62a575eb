/* warp.hip -- ring frames resampled at displaced positions (beamformer_hip_warp_last_frames): one launch.  include/ogl_beamformer_hip.h
 * has the definition for callers, operation for operation; tests/warp_ref.py restates it in numpy.
 *
 * warp_kernel.  A block of 256 lanes owns a tile of one frame -- 2^tile_log2[a] voxels an axis (bf_warp_tile: 8 x 8 x 4 in a volume,
 * 16 x 16 on a plane; fewer than 256 voxels where the frame is smaller: the lanes beyond idle) --, a lane one output voxel.
 * PHASE 1.  Every lane interpolates its displacement from the call's table (the nodes around it: L1 / L2; a rigid shift is one
 * broadcast load a component), forms its position, its first tap index and its weights per axis, and the block reduces the lowest and
 * the highest source index any lane reads, per axis (wave shuffles, then 24 words of LDS: no atomics).  The indices are kept BIASED
 * by kBias = 4 in uint32 -- index + 4 --: a position is first clamped to -3 .. extent + 1 (beyond which every tap lies outside the
 * frame, or at the clamped edge, either way), so a biased index lies in 0 .. 2^31 + 7 and no frame of up to 2^31 - 1 points an axis
 * overflows anything.
 * PHASE 2, the STAGED path (the smooth fields that motion produces).  The box of source voxels between those ends -- the tile, the
 * support and what the displacement varies by across the tile --, cut to the frame, is staged once in LDS in flat order, rows
 * contiguous; the taps then come from LDS.  The edge is handled by the tap, not by the staging: a Zero-mode term outside the frame
 * is skipped by the same test on either path, a Clamp-mode index is clamped before it is used, so every address lies inside the
 * box and the box inside the frame.
 * The DIRECT path (a wild field: the box holds more than BF_WARP_BOX_VOXELS voxels; or args.direct) reads the same voxels from the
 * ring through L1 / L2.  Both paths run ONE text, sample(), under two fetches: the arithmetic, its order and therefore the bytes are
 * the same, and an output does not depend on what else shares its tile.
 *
 * LDS: BF_WARP_BOX_VOXELS voxels -- 32 KiB (complex), 16 KiB (real) -- and 96 bytes of ends: four blocks fit the 160 KiB of a CU.
 * Eight instantiations: kind x interpolation x edge; which axes have one point is a uniform branch.  No atomics, no scratch memory;
 * __launch_bounds__ is the launch's block size. */
#include <hip/hip_runtime.h>
#include "bf_kernels.h"

typedef float warp_f32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr uint32_t kBias = 4u;

template <bool CPLX> struct Voxel;
template <> struct Voxel<true>  { typedef warp_f32x2 type; };
template <> struct Voxel<false> { typedef float type; };

__device__ __forceinline__ float zero_of(float)            { return 0.0f; }
__device__ __forceinline__ warp_f32x2 zero_of(warp_f32x2)  { warp_f32x2 z; z.x = 0.0f; z.y = 0.0f; return z; }
__device__ __forceinline__ float term(float w, float v, float acc) { return __builtin_fmaf(w, v, acc); }
__device__ __forceinline__ warp_f32x2 term(float w, warp_f32x2 v, warp_f32x2 acc)
{
	acc.x = __builtin_fmaf(w, v.x, acc.x); acc.y = __builtin_fmaf(w, v.y, acc.y);
	return acc;
}
/* the mix's chains for a one-term product (mix_term.h) */
__device__ __forceinline__ float rotated(float v, float re, float) { return __builtin_fmaf(re, v, 0.0f); }
__device__ __forceinline__ warp_f32x2 rotated(warp_f32x2 v, float re, float im)
{
	warp_f32x2 o;
	o.x = __builtin_fmaf(re, v.x, 0.0f); o.x = __builtin_fmaf(-im, v.y, o.x);
	o.y = __builtin_fmaf(im, v.x, 0.0f); o.y = __builtin_fmaf(re, v.y, o.y);
	return o;
}

/* one component of the displacement at lattice cell j, fractions s: the lerps along x, then y, then z; node: the frame's value at
 * node (j[0], j[1], j[2]) for this component, N the lattice */
__device__ __forceinline__ float lattice_value(const float *__restrict__ node, const uint32_t (&N)[3], const float (&s)[3])
{
	const auto along_x = [&](uint32_t dy, uint32_t dz) {
		const float *q = node + ((size_t)dz * N[1] + dy) * N[0] * 3u;
		float lo = q[0];
		if (N[0] > 1u) lo = __builtin_fmaf(s[0], q[3] - lo, lo);
		return lo;
	};
	const auto along_y = [&](uint32_t dz) {
		float lo = along_x(0u, dz);
		if (N[1] > 1u) lo = __builtin_fmaf(s[1], along_x(1u, dz) - lo, lo);
		return lo;
	};
	float lo = along_y(0u);
	if (N[2] > 1u) lo = __builtin_fmaf(s[2], along_y(1u) - lo, lo);
	return lo;
}

/* the separable sum of one output voxel: off[a][t] the tap's share of the address, ok[a] bit t: the term is taken */
template <class T, uint32_t NT, class Fetch>
__device__ __forceinline__ T sample(const uint32_t (&off)[3][NT], const uint32_t (&ok)[3], const float (&w)[3][NT], const uint32_t (&taps)[3], Fetch fetch)
{
	T az = zero_of(T());
	#pragma unroll
	for (uint32_t tz = 0; tz < NT; tz++) {
		if (tz >= taps[2] || !(ok[2] >> tz & 1u)) continue;
		T ay = zero_of(T());
		#pragma unroll
		for (uint32_t ty = 0; ty < NT; ty++) {
			if (ty >= taps[1] || !(ok[1] >> ty & 1u)) continue;
			T ax = zero_of(T());
			#pragma unroll
			for (uint32_t tx = 0; tx < NT; tx++) {
				if (tx >= taps[0] || !(ok[0] >> tx & 1u)) continue;
				ax = term(w[0][tx], fetch(off[0][tx] + off[1][ty] + off[2][tz]), ax);
			}
			ay = term(w[1][ty], ax, ay);
		}
		az = term(w[2][tz], ay, az);
	}
	return az;
}

} // namespace

template <bool CPLX, bool CUBIC, bool CLAMP>
__global__ __launch_bounds__(BF_WARP_THREADS) void warp_kernel(char *__restrict__ ring, const uint64_t *__restrict__ offsets,
                                                               const float *__restrict__ table, BfWarpArgs a)
{
	typedef typename Voxel<CPLX>::type T;
	constexpr uint32_t NT = CUBIC ? 4u : 2u;
	__shared__ T box[BF_WARP_BOX_VOXELS];
	__shared__ uint32_t ends[BF_WARP_THREADS / 64u][6];

	uint32_t b = blockIdx.x, tile[3];
	tile[0] = b % a.tiles[0]; b /= a.tiles[0];
	tile[1] = b % a.tiles[1]; b /= a.tiles[1];
	tile[2] = b % a.tiles[2];
	const uint32_t n = b / a.tiles[2];                       /* the frame */
	uint32_t v[3], l = threadIdx.x;
	bool active = true;
	#pragma unroll
	for (uint32_t k = 0; k < 3; k++) {
		v[k] = (tile[k] << a.tile_log2[k]) + (l & ((1u << a.tile_log2[k]) - 1u));
		l >>= a.tile_log2[k];
		active = active && v[k] < a.points[k];
	}
	active = active && l == 0u;                              /* a tile of fewer than 256 voxels (bf_warp_tile): the lanes beyond it idle */

	/* ---- phase 1: the lane's displacement, position, first tap and weights; the block's ends ---- */
	const uint32_t N[3] = {a.nodes[0], a.nodes[1], a.nodes[2]};
	uint32_t first[3] = {kBias, kBias, kBias}, taps[3] = {1u, 1u, 1u};   /* an axis of one point: one tap at index 0 of weight 1 */
	float w[3][NT];
	#pragma unroll
	for (uint32_t k = 0; k < 3; k++) {
		w[k][0] = 1.0f;
		#pragma unroll
		for (uint32_t t = 1; t < NT; t++) w[k][t] = 0.0f;
	}
	uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
	if (active) {
		uint32_t j[3] = {0u, 0u, 0u};
		float s[3] = {0.0f, 0.0f, 0.0f};
		#pragma unroll
		for (uint32_t k = 0; k < 3; k++) {
			if (N[k] > 1u) {
				float c = ((float)v[k] - a.node_first[k]) * a.inv_step[k];
				c = __builtin_fminf(__builtin_fmaxf(c, 0.0f), (float)(N[k] - 1u));
				const uint32_t cell = (uint32_t)__builtin_floorf(c);
				j[k] = cell < N[k] - 2u ? cell : N[k] - 2u;
				s[k] = c - (float)j[k];
			}
		}
		const float *node = table + 2u * a.frames + (((size_t)n * N[2] + j[2]) * N[1] + j[1]) * N[0] * 3u + (size_t)j[0] * 3u;
		#pragma unroll
		for (uint32_t k = 0; k < 3; k++) {
			if (a.points[k] > 1u) {
				const float d = lattice_value(node + k, N, s);
				const float p = (float)v[k] + d;
				const float fi = __builtin_floorf(p);
				const float t = p - fi;
				long long i = (long long)fi;
				const long long top = (long long)a.points[k] + 1;
				i = i < -3 ? -3 : (i > top ? top : i);
				taps[k] = NT;
				if (CUBIC) {
					first[k] = (uint32_t)(i - 1 + (long long)kBias);
					w[k][0] = __builtin_fmaf(__builtin_fmaf(-0.5f, t, 1.0f), t, -0.5f) * t;
					w[k][1] = __builtin_fmaf(__builtin_fmaf(1.5f, t, -2.5f) * t, t, 1.0f);
					w[k][2] = __builtin_fmaf(__builtin_fmaf(-1.5f, t, 2.0f), t, 0.5f) * t;
					w[k][3] = (__builtin_fmaf(0.5f, t, -0.5f) * t) * t;
				} else {
					first[k] = (uint32_t)(i + (long long)kBias);
					w[k][0] = 1.0f - t;
					w[k][1] = t;
				}
			}
		}
		#pragma unroll
		for (uint32_t k = 0; k < 3; k++) {
			const uint32_t bottom = kBias, top = a.points[k] - 1u + kBias, last = first[k] + taps[k] - 1u;
			lo[k] = first[k] < bottom ? bottom : (first[k] > top ? top : first[k]);
			hi[k] = last < bottom ? bottom : (last > top ? top : last);
		}
	}
	#pragma unroll
	for (uint32_t k = 0; k < 3; k++) {
		#pragma unroll
		for (uint32_t m = 32u; m; m >>= 1) {
			const uint32_t other_lo = (uint32_t)__shfl_xor((int)lo[k], (int)m, 64), other_hi = (uint32_t)__shfl_xor((int)hi[k], (int)m, 64);
			lo[k] = other_lo < lo[k] ? other_lo : lo[k];
			hi[k] = other_hi > hi[k] ? other_hi : hi[k];
		}
	}
	if ((threadIdx.x & 63u) == 0u) {
		#pragma unroll
		for (uint32_t k = 0; k < 3; k++) { ends[threadIdx.x >> 6][k] = lo[k]; ends[threadIdx.x >> 6][3u + k] = hi[k]; }
	}
	__syncthreads();
	uint32_t origin[3], extent[3];
	#pragma unroll
	for (uint32_t k = 0; k < 3; k++) {
		uint32_t low = ends[0][k], high = ends[0][3u + k];
		#pragma unroll
		for (uint32_t wave = 1; wave < BF_WARP_THREADS / 64u; wave++) {
			low = ends[wave][k] < low ? ends[wave][k] : low;
			high = ends[wave][3u + k] > high ? ends[wave][3u + k] : high;
		}
		origin[k] = __builtin_amdgcn_readfirstlane(low);           /* (a tile has an active lane: low <= high, both inside the frame) */
		extent[k] = __builtin_amdgcn_readfirstlane(high) - origin[k] + 1u;
	}
	const bool staged = !a.direct && extent[0] <= BF_WARP_BOX_VOXELS && extent[1] <= BF_WARP_BOX_VOXELS && extent[2] <= BF_WARP_BOX_VOXELS &&
	                    (uint64_t)extent[0] * extent[1] * extent[2] <= BF_WARP_BOX_VOXELS;

	/* ---- phase 2: the box into LDS (staged), then the taps ---- */
	const T *src = (const T *)(ring + offsets[n]);
	const uint32_t nx = a.points[0], nxy = a.points[0] * a.points[1];   /* (a frame holds less than 2^31 voxels) */
	if (staged) {
		const uint32_t total = extent[0] * extent[1] * extent[2];
		const uint32_t corner = ((origin[2] - kBias) * a.points[1] + (origin[1] - kBias)) * nx + (origin[0] - kBias);
		for (uint32_t q = threadIdx.x; q < total; q += BF_WARP_THREADS) {
			const uint32_t row = q / extent[0], x = q - row * extent[0];
			const uint32_t z = row / extent[1], y = row - z * extent[1];
			box[q] = src[corner + z * nxy + y * nx + x];
		}
		__syncthreads();
	}
	if (!active) return;

	const uint32_t base[3] = {staged ? origin[0] : kBias, staged ? origin[1] : kBias, staged ? origin[2] : kBias};
	const uint32_t stride[3] = {1u, staged ? extent[0] : nx, staged ? extent[0] * extent[1] : nxy};
	uint32_t off[3][NT], ok[3];
	#pragma unroll
	for (uint32_t k = 0; k < 3; k++) {
		ok[k] = 0u;
		const uint32_t bottom = kBias, top = a.points[k] - 1u + kBias;
		#pragma unroll
		for (uint32_t t = 0; t < NT; t++) {
			const uint32_t u = first[k] + t;
			const uint32_t inside = u < bottom ? bottom : (u > top ? top : u);
			if (CLAMP || inside == u) ok[k] |= 1u << t;
			off[k][t] = (inside - base[k]) * stride[k];
		}
	}
	T out;
	if (staged) out = sample<T, NT>(off, ok, w, taps, [&](uint32_t at) { return box[at]; });
	else        out = sample<T, NT>(off, ok, w, taps, [&](uint32_t at) { return src[at]; });
	if (a.rotate) out = rotated(out, table[2u * n], table[2u * n + 1u]);
	T *dst = (T *)(ring + a.out_offset + (uint64_t)n * a.out_stride);
	dst[v[2] * nxy + v[1] * nx + v[0]] = out;
}

namespace {

template <bool CPLX, bool CUBIC>
hipError_t launch(void *ring, const uint64_t *offsets, const float *table, const BfWarpArgs &a, uint32_t blocks, hipStream_t s)
{
	if (a.clamp) hipLaunchKernelGGL((warp_kernel<CPLX, CUBIC, true>), dim3(blocks), dim3(BF_WARP_THREADS), 0, s, (char *)ring, offsets, table, a);
	else         hipLaunchKernelGGL((warp_kernel<CPLX, CUBIC, false>), dim3(blocks), dim3(BF_WARP_THREADS), 0, s, (char *)ring, offsets, table, a);
	return hipGetLastError();
}

} // namespace

/* One launch.  The sources, the output run and the table are device memory and do not overlap: the caller's business (frame_ops.cpp:
 * warp_last_frames), nothing here re-checks it.  The launch geometry in `args` is filled in here. */
extern "C" hipError_t bf_launch_warp(void *ring, const uint64_t *offsets, const float *table, const BfWarpArgs *args, hipStream_t s)
{
	if (!ring || !offsets || !table || !args) return hipErrorInvalidValue;
	BfWarpArgs a = *args;
	uint64_t voxels = 1, node_product = 1, blocks = a.frames;
	for (uint32_t k = 0; k < 3; k++) {
		if (a.points[k] == 0 || a.nodes[k] == 0) return hipErrorInvalidValue;
		voxels *= a.points[k];
		node_product *= a.nodes[k];
		if (voxels > 0x7FFFFFFFull || node_product > BF_WARP_MAX_NODES) return hipErrorInvalidValue;
	}
	if (a.frames == 0 || a.frames > BF_ENSEMBLE_MAX_FRAMES || a.frames * node_product > BF_WARP_MAX_ENTRIES || a.cubic > 1u || a.clamp > 1u)
		return hipErrorInvalidValue;
	bf_warp_tile(a.points, a.tile_log2);
	for (uint32_t k = 0; k < 3; k++) {
		a.tiles[k] = (uint32_t)(((uint64_t)a.points[k] + (1u << a.tile_log2[k]) - 1u) >> a.tile_log2[k]);
		blocks *= a.tiles[k];
		if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
	}
	const uint32_t g = (uint32_t)blocks;
	if (a.cplx) return a.cubic ? launch<true, true>(ring, offsets, table, a, g, s) : launch<true, false>(ring, offsets, table, a, g, s);
	return a.cubic ? launch<false, true>(ring, offsets, table, a, g, s) : launch<false, false>(ring, offsets, table, a, g, s);
}
