/* readi_decode.hip -- the READI image's decode ACROSS acquisitions, for gfx950.
 *
 * shaders/das.glsl:288-366: READI_FORCES is FORCES with transmit element tx_group * AcquisitionCount + tx_event and every term
 * multiplied by Hadamard[readi_group * G + tx_group].  Everything behind that factor is linear in the samples, so the sum of the N
 * partial frames of a READI sequence (RF k under group g_k) is ONE FORCES frame of
 *     D[channel][t * A + event][sample] = sum over k of H[g_k][t] * rf_k[channel][event][sample],      t < G,
 * which is what this kernel writes.  Bandwidth bound: N * C * A * S samples in, C * G * A * S out, one multiply-add per (k, t, sample).
 *
 * A channel's [event][sample] slab is contiguous on both sides, so a thread takes 16 bytes of a slab (complex samples are two floats:
 * one body for both kinds), reads them once per RF frame and keeps one accumulator per t of its tile of TILE groups; G up to 256 is
 * covered by tiling t over grid z (TILE divides G: Hadamard orders are 2 or multiples of 4).  The group of frame k and the signs of
 * its row come through wave-uniform (scalar) loads: k, the tile and the table pointers (restrict parameters: nothing the kernel
 * writes) are the same in every lane.
 *
 * The sum is fixed: float32, acc = fma(x, +-1, acc) for k = 0, 1, ... N - 1 from +0 -- acc +- x with one rounding, bit for bit what a
 * sequential float32 loop on the host gives (tests/test_gpu_readi_image.py compares the buffer as words).
 */
#include <hip/hip_runtime.h>
#include "bf_kernels.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename V> struct lanes_of        { static constexpr uint32_t value = 1; };
template <>           struct lanes_of<f32x4> { static constexpr uint32_t value = 4; };

template <typename V, int TILE>
__global__ __launch_bounds__(256) void readi_image_decode_kernel(const BfReadiDecodeArgs a, const uint32_t *const __restrict__ groups,
                                                                 const uint32_t *const __restrict__ hadamard)
{
	const uint32_t G = a.group_count, channel = blockIdx.y, t0 = blockIdx.z * TILE;
	const uint64_t n = a.slab_floats / lanes_of<V>::value;                 /* V's per slab */
	const V *in  = (const V *)a.in + (uint64_t)channel * n;
	V       *out = (V *)a.out + ((uint64_t)channel * G + t0) * n;
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
		V acc[TILE];
		#pragma unroll
		for (int t = 0; t < TILE; t++) acc[t] = V(0.0f);
		for (uint32_t k = 0; k < a.frames; k++) {
			const V x = ((const V *)((const char *)in + a.in_frame_bytes * k))[i];
			/* row groups[k], entries t0 .. t0 + TILE: an even index (G and TILE are even), TILE / 2 whole words */
			const uint32_t *row = hadamard + (((uint64_t)groups[k] * G + t0) >> 1);
			#pragma unroll
			for (int t = 0; t < TILE; t++) {
				const uint32_t half = row[t >> 1] >> (16 * (t & 1));
				const float sign = __uint_as_float(((half & 0x8000u) << 16) | 0x3F800000u);      /* binary16 +-1 -> float32 +-1 */
				acc[t] = __builtin_elementwise_fma(x, V(sign), acc[t]);
			}
		}
		#pragma unroll
		for (int t = 0; t < TILE; t++) out[(uint64_t)t * n + i] = acc[t];
	}
}

template <typename V, int TILE>
static hipError_t launch_tile(const BfReadiDecodeArgs *a, hipStream_t s)
{
	const uint64_t n = a->slab_floats / lanes_of<V>::value, blocks = (n + 255) / 256;
	const dim3 grid((uint32_t)(blocks < 65535u ? blocks : 65535u), a->channels, a->group_count / TILE);
	hipLaunchKernelGGL((readi_image_decode_kernel<V, TILE>), grid, dim3(256), 0, s, *a, a->groups, a->hadamard);
	return hipGetLastError();
}

template <typename V>
static hipError_t launch_decode(const BfReadiDecodeArgs *a, hipStream_t s)
{
	const uint32_t G = a->group_count;
	return G % 16 == 0 ? launch_tile<V, 16>(a, s) : G % 12 == 0 ? launch_tile<V, 12>(a, s) : G % 8 == 0 ? launch_tile<V, 8>(a, s)
	     : G % 4 == 0  ? launch_tile<V, 4>(a, s)  : launch_tile<V, 2>(a, s);
}

/* group_count: an order the host's Hadamard construction has -- 2 or a multiple of 4 --, at most BeamformerMaxEmissionsCount;
 * channels <= BeamformerMaxChannelCount: grid y and z stay far under 65535, grid x is capped there and strided */
extern "C" hipError_t bf_launch_readi_image_decode(const BfReadiDecodeArgs *a, hipStream_t s)
{
	if (!a->frames || !a->channels || !a->slab_floats) return hipSuccess;
	if (a->group_count < 2 || (a->group_count & 1)) return hipErrorInvalidValue;
	/* 16-byte accesses where every slab starts on 16 bytes (the frames do: their strides are multiples of 64) */
	return a->slab_floats % 4 == 0 ? launch_decode<f32x4>(a, s) : launch_decode<float>(a, s);
}
