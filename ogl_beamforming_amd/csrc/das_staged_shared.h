/* das_staged_shared.h -- the tile set-up of the row-column DAS family, once: block id -> tile, the transmit index of a table entry,
 * the tile-wide extremes of the transmit delays, window-relative table rows, the receive table of a channel chunk, the staging
 * offsets and loads, thread -> voxel, the store, and the host's launch and shape dispatch.  das_staged.hip (staged_body and
 * staged_tables_kernel; the channel-paired body keeps its own hand-placed prologue), das_staged_real.hip and das_separable.hip
 * call these (the gather kernel all but the transmit index, which it keeps as text: it says why); their inner loops stay in their
 * files.  das_staged_cubic.hip shares the host code, the row helper and the store and keeps the rest of this arithmetic as text: built
 * from these calls it was measurably slower (it says by how much).  Nothing here branches at run time on its caller: what
 * differs between the kernels is a template parameter.
 */
#ifndef BF_DAS_STAGED_SHARED_H
#define BF_DAS_STAGED_SHARED_H

#include "das_common.h"

typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) f32x2 lds_f32x2;
typedef __attribute__((address_space(3))) f32x4 lds_f32x4;

/* The block's tile: blockIdx -> tile with each XCD walking a contiguous run of tiles (das.hip), then the walk order of the tile list.
 * Depth-major (q.depth_major & DEPTH_MASK; the staged kernels test bit 0, the gather kernel every bit): consecutive tiles -- the
 * ones an XCD has in flight together -- are a few columns adjacent along u at consecutive depths, whose RF windows overlap (the
 * window moves ~1.5 samples per plane and ~14 per tile laterally at config 4), so the lines one tile pulls into the XCD's L2 serve
 * its neighbours (bf_column_walk, bf_kernels.h).  Plane-major: x, then y, then z.
 * depth_major bit 2 (global transmit tables): planes in chunks of 32, so that blocks j and j + 32 of an XCD's
 * sequence -- the two a CU holds (dispatch is breadth first over an XCD's 32 CUs) -- are NEIGHBOURS ALONG u in one plane: they read
 * the same rows of the global transmit table (14.6 KB at 76 transmits: the scalar cache holds 16 KB) and adjacent RF windows.
 * tu, tv, zl: along the receive axis, along the transmit axis, plane inside the shard.
 * False: no tile (the grid's rounding, the last chunk's padding) -- a whole block: no barrier is skipped.
 * (One of six copies of the walk; tests/walk_cases.py pins each at the tile, column and z-chunk counts where its branches differ.) */
template <uint32_t DEPTH_MASK = 1u>
__device__ __forceinline__ bool staged_tile_of(const BfSeparableArgs &q, bool global_tables, uint32_t &tu, uint32_t &tv, uint32_t &zl)
{
	const bool paired = global_tables && (q.depth_major & 4u);
	const uint32_t zchunks = (q.tiles[2] + 31u) >> 5;
	const uint32_t total = paired ? q.tiles[0] * q.tiles[1] * zchunks * 32u : q.tiles[0] * q.tiles[1] * q.tiles[2];
	const uint32_t per   = (total + 7u) / 8u;
	const uint32_t tile  = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
	if (tile >= total) return false;
	if (paired) {
		uint32_t r = tile >> 5;
		tu = r % q.tiles[0]; r /= q.tiles[0];
		zl = (r % zchunks) * 32u + (tile & 31u);
		tv = r / zchunks;
		return zl < q.tiles[2];
	}
	if (q.depth_major & DEPTH_MASK) {
		bf_column_walk(tile, q.tiles[0], q.tiles[2], q.walk_columns, tu, tv, zl);
	} else {
		tu = tile % q.tiles[0];
		tv = (tile / q.tiles[0]) % q.tiles[1];
		zl = tile / (q.tiles[0] * q.tiles[1]);
	}
	return true;
}

/* absolute sample index of transmit a's delay to the voxels at normalised coordinate v_coord along the transmit lateral axis, plane pz */
__device__ __forceinline__ float rca_transmit_index(const BfDasArgs &p, uint32_t a, uint32_t v_axis, float v_coord, float pz)
{
	float coord[3] = {0.f, 0.f, pz};
	coord[v_axis] = v_coord;
	float wx, wy, wz;
	m4_point(p.voxel_transform, coord[0], coord[1], coord[2], wx, wy, wz);
	const BfTransmit t = p.transmits[a];
	float dist = 0.f;
	if (!(t.flags & BF_TX_NONE)) {
		float px = (t.flags & BF_TX_ROWS) ? wy : wx;
		if (t.flags & BF_TX_PLANE) dist = px * t.sin_a + wz * t.cos_a;
		else { float ddx = px - t.focus_x, ddz = wz - t.focus_z; dist = hw_sqrt(ddx * ddx + ddz * ddz); }
	}
	return (div_speed_of_sound(dist, p) + p.time_offset) * p.sampling_frequency;
}

/* ---- transmit tables of tile row tv on plane z (absolute delays first): put(a, iv, e, t_index, cos, sin) for every entry
 * e = a * V + iv of A4 transmits (the count rounded up to a multiple of 4) x V lateral rows, in the caller's own layout */
template <int VS, bool PHASOR, typename Put>
__device__ __forceinline__ void staged_transmit_entries(const BfDasArgs &p, uint32_t v_axis, uint32_t tv, uint32_t z, uint32_t tid, uint32_t nthreads, Put &&put)
{
	constexpr uint32_t V = 1u << VS;
	const int A = p.acquisition_count, A4 = (A + 3) & ~3;
	const float denom_v = fmaxf(1.0f, (float)p.size[v_axis] - 1.0f);
	const float pz = (float)z / fmaxf(1.0f, (float)p.size[2] - 1.0f);
	const float phase_k = p.demodulation_frequency * p.inv_sampling_frequency;
	for (uint32_t e = tid; e < (uint32_t)A4 * V; e += nthreads) {
		uint32_t a = e >> VS, iv = e & (V - 1);
		float cs_c = 0.f, cs_s = 0.f, t_idx = 0.f;           /* padding transmits: zero phasor, window position 0 (over a zero row) */
		if (a < (uint32_t)A) {
			t_idx = rca_transmit_index(p, a, v_axis, (float)(tv * V + iv) / denom_v, pz);
			if constexpr (PHASOR) {
				float turns = phase_turns(phase_k, t_idx);
				cs_c = hw_cos_turns(turns); cs_s = hw_sin_turns(turns);
			}
		}
		put(a, iv, e, t_idx, cs_c, cs_s);
	}
}

/* the same for every lane: keep it in scalar registers.  (Through scalar temporaries: __builtin_bit_cast applied
 * directly to a vector component reads the vector's FIRST component with this hipcc -- range.y silently became
 * range.x, and waves whose lanes reach the end of the RF row for the tile's largest transmit delay only took the
 * unchecked loop; found by the focused-transmit parity case, whose delays differ by hundreds of samples.) */
__device__ __forceinline__ f32x2 staged_uniform_range(f32x2 range)
{
	const float lo = range.x, hi = range.y;
	range.x = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, lo)));
	range.y = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, hi)));
	return range;
}

/* tile-wide extremes {min, max} of the absolute transmit delay (for the range-test shortcut): every wave reduces its share of the
 * `count` table entries delay_of(e), the block combines the per-wave results through wave_range[waves of the block].  The staged
 * kernels keep wave_range in their dynamic LDS (they must have NO static LDS in front of it: their tap address arithmetic depends
 * on it), the gather kernel in static LDS.  (threadIdx.x and blockDim.x are read here, where they are used, and not handed in as
 * values: as arguments they cost every instance of the gather kernel two VGPRs.) */
template <typename DelayOf>
__device__ __forceinline__ f32x2 rca_tile_range(uint32_t count, f32x2 *wave_range, DelayOf &&delay_of)
{
	__syncthreads();
	{
		float lo = __builtin_inff(), hi = -__builtin_inff();
		for (uint32_t e = threadIdx.x; e < count; e += blockDim.x) {
			float v = delay_of(e);
			lo = fminf(lo, v); hi = fmaxf(hi, v);
		}
		for (int off = 32; off > 0; off >>= 1) {
			lo = fminf(lo, __shfl_xor(lo, off, 64));
			hi = fmaxf(hi, __shfl_xor(hi, off, 64));
		}
		if ((threadIdx.x & 63u) == 0) wave_range[threadIdx.x >> 6] = f32x2{lo, hi};
	}
	__syncthreads();
	f32x2 range = wave_range[0];
	for (uint32_t w = 1; w < (blockDim.x >> 6); w++) {
		range.x = fminf(range.x, wave_range[w].x);
		range.y = fmaxf(range.y, wave_range[w].y);
	}
	return staged_uniform_range(range);
}

/* per transmit: floor of the smallest delay of its table row, returned; the row (V floats, STRIDE floats apart) becomes
 * window-relative, T'' = T - floor - 1/2, or + 1/2 where the window starts one sample early (LEAD = 1: the cubic kernel's tap k - 1) */
template <uint32_t V, uint32_t STRIDE, int LEAD>
__device__ __forceinline__ int staged_window_row(float *row)
{
	float m = row[0];
	#pragma unroll 4
	for (uint32_t iv = 1; iv < V; iv++) m = fminf(m, row[STRIDE * iv]);
	float fl = __builtin_floorf(m);
	#pragma unroll 4
	for (uint32_t iv = 0; iv < V; iv++) {
		if constexpr (LEAD) row[STRIDE * iv] = (row[STRIDE * iv] - fl) + 0.5f;      /* both steps exact */
		else                row[STRIDE * iv] = (row[STRIDE * iv] - fl) - 0.5f;
	}
	return (int)fl;
}

/* ---- the receive table of channels [c0, c0 + cn) for tile column tu, rebuilt once per chunk of channels from ~50 scalars of the
 * launch arguments (two 4 x 4 transforms, pitch, f-number, speed of sound, ...).  Held in SGPRs across the channel loop they cost the
 * complex kernel 140 scalar spills (v_writelane / v_readlane into two of its 64 VGPRs, which in turn pushed 5 vector registers to
 * scratch: 3.4 GiB written per 1 GiB frame).  They are read from the kernel-argument segment instead, through a pointer the compiler
 * cannot see through, at the top of every chunk: a few s_load per 16 channels, dead again before the channel loop.
 * Entry f32x4: { R', apod*cos(phi_r), apod*sin(phi_r), +-apod };  f32x2 (real samples): { R', +-apod }.
 * LEAD: samples the interpolation needs in front of floor(index) -- the range is [LEAD, S - 1 - LEAD) (das.glsl: linear
 * 0 <= index < S - 1, cubic 1 <= index < S - 2).  Leaves with a barrier behind the finished table. */
template <typename Entry, int LEAD>
__device__ __forceinline__ void staged_receive_table(Entry *R, int *rfloor, int c0, int cn, uint32_t tu, uint32_t z, uint32_t u_axis, uint32_t u_shift,
                                                     bool rx_rows, f32x2 range, int S, uint32_t tid, uint32_t nthreads)
{
	constexpr int WEIGHT = sizeof(Entry) / 4 - 1, FLOATS = sizeof(Entry) / 4;
	const uint32_t U = 1u << u_shift;
	{
	typedef __attribute__((address_space(4))) const BfDasArgs const_args;
	const_args *ka = (const_args *)__builtin_amdgcn_kernarg_segment_ptr();
	static_assert(__builtin_offsetof(BfDasArgs, xdc_transform) == 0, "BfDasArgs is the kernel's first argument: it sits at offset 0 of the segment");
	asm volatile("" : "+s"(ka));
	const uint32_t k_size[3] = {ka->size[0], ka->size[1], ka->size[2]};
	const float k_denom_u = fmaxf(1.0f, (float)k_size[u_axis] - 1.0f);
	const float k_pz = (float)z / fmaxf(1.0f, (float)k_size[2] - 1.0f);
	const float k_fs = ka->sampling_frequency, k_inv_c = ka->inv_speed_of_sound, k_c = ka->speed_of_sound, k_fnum = ka->f_number;
	[[maybe_unused]] const float k_phase = ka->demodulation_frequency * ka->inv_sampling_frequency;
	const float k_pitch = rx_rows ? ka->pitch[1] : ka->pitch[0];
	for (uint32_t e = tid; e < (uint32_t)cn * U; e += nthreads) {
		uint32_t c = (uint32_t)c0 + (e >> u_shift), iu = e & (U - 1);
		float coord[3] = {0.f, 0.f, k_pz};
		coord[u_axis] = (float)(tu * U + iu) / k_denom_u;
		float wx, wy, wz, xx, xy, xz;
		m4_point(ka->voxel_transform, coord[0], coord[1], coord[2], wx, wy, wz);
		m4_point(ka->xdc_transform, wx, wy, wz, xx, xy, xz);
		float lateral = rx_rows ? xy : xx;
		float dx      = lateral - (float)c * k_pitch;
		float a_arg   = __builtin_fabsf(dx * (k_fnum * hw_rcp(__builtin_fabsf(xz))));
		/* the delay is kept for lanes outside the aperture too: it keeps their (discarded)
		 * LDS reads inside the window */
		float r_idx = div_speed_of_sound(hw_sqrt(dx * dx + xz * xz), k_inv_c, k_c) * k_fs;
		Entry entry = {};
		entry[0] = r_idx;
		if (a_arg < 0.5f) {
			float cs    = hw_cos_turns(0.5f * a_arg);
			float apod  = cs * cs;
			if constexpr (FLOATS == 4) {
				float turns = phase_turns(k_phase, r_idx);
				entry[1] = apod * hw_cos_turns(turns);
				entry[2] = apod * hw_sin_turns(turns);
			}
			entry[WEIGHT] = apod;
		}
		R[e] = entry;
	}
	}
	__syncthreads();
	for (uint32_t cl = tid; cl < (uint32_t)cn; cl += nthreads) {
		const float *row = reinterpret_cast<const float *>(R + (size_t)cl * U);
		float m = row[0];
		#pragma unroll 4
		for (uint32_t iu = 1; iu < U; iu++) m = fminf(m, row[FLOATS * iu]);
		rfloor[cl] = (int)__builtin_floorf(m);
	}
	__syncthreads();
	/* the entries become what the channel loop consumes with no arithmetic: the delay relative to the channel's window
	 * (exact) and, in the SIGN of the weight, whether the lane can leave the RF row for some transmit of the tile
	 * (linear: r + min T < 0 or r + max T >= S - 1: such a wave runs the checked loop) */
	for (uint32_t e = tid; e < (uint32_t)cn * U; e += nthreads) {
		Entry entry = R[e];
		const bool lane_safe = (entry[0] + range.x >= (float)LEAD) && (entry[0] + range.y < (float)(S - 1 - LEAD));
		entry[0] -= (float)rfloor[e >> u_shift];
		if (!lane_safe) entry[WEIGHT] = -entry[WEIGHT];          /* -0.0f for a lane outside the aperture: still "unsafe" to the sign test */
		R[e] = entry;
	}
	__syncthreads();
}

/* ---- Staging.  Thread tid copies element j = tid % W of windows a_n = tid / W + n * (threads / W), n < NL:
 * sample rfl + floor(tmin_a) - LEAD + j of row (channel, a).  The loads are buffer loads over the whole DAS
 * input: an offset outside it (a window that starts before the first row or ends behind the last)
 * returns zero instead of faulting, and samples a window holds from a NEIGHBOURING row are never
 * consumed -- a term is only evaluated (unchecked loop) or only kept (checked loop) when all of
 * its taps lie inside its own row.  Per thread and n one loop-invariant byte offset; per channel one add.
 * Sample: f32x2 (complex) or float. */
template <typename Sample>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t staged_rf_resource(const BfDasArgs &p)
{
	return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.rf), 0,
		(int)((uint32_t)p.channel_count * (uint32_t)p.acquisition_count * (uint32_t)p.sample_count * (uint32_t)sizeof(Sample)), 0x00020000);
}
template <typename Sample, int WS, int LEAD, int NL>
__device__ __forceinline__ void staged_stage_offsets(uint32_t (&stage_inv)[NL], const int *tfl, int A, int S, uint32_t tid, uint32_t nthreads)
{
	constexpr uint32_t W = 1u << WS;
	const uint32_t windows_per_pass = nthreads >> WS;
	#pragma unroll
	for (int n = 0; n < NL; n++) {
		uint32_t a = (tid >> WS) + (uint32_t)n * windows_per_pass;
		/* transmits of the padding (a >= A) point far outside the buffer: they stage zeros */
		stage_inv[n] = a < (uint32_t)A ? (a * (uint32_t)S + (uint32_t)(tfl[a] - LEAD + (int)(tid & (W - 1)))) * (uint32_t)sizeof(Sample) : 0x80000000u;
	}
}
template <typename Sample, int NL>
__device__ __forceinline__ void staged_stage_load(__amdgpu_buffer_rsrc_t rf_rsrc, const uint32_t (&stage_inv)[NL], int channel, int A, int S, int rfl, Sample (&regs)[NL])
{
	const uint32_t at = ((uint32_t)channel * (uint32_t)A * (uint32_t)S + (uint32_t)rfl) * (uint32_t)sizeof(Sample);
	#pragma unroll
	for (int n = 0; n < NL; n++) {
		/* (the padding's 0x80000000 + at stays out of range: the host refuses inputs of 2 GiB and more here) */
		if constexpr (sizeof(Sample) == 8) {
			i32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rf_rsrc, (int)(stage_inv[n] + at), 0, 0);
			regs[n] = __builtin_bit_cast(f32x2, v);
		} else {
			regs[n] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rf_rsrc, (int)(stage_inv[n] + at), 0, 0));
		}
	}
}

/* thread -> voxel: lanes run along the output's x axis.  lane_u, lane_v: the thread's place in the U x V tile (the extents AND their
 * shifts, as the caller already holds them: formed again from the shifts here, the uniform-table instances of the complex kernel
 * took four more VGPRs and the gather kernel's cubic ones spilled) */
__device__ __forceinline__ void rca_voxel_of(uint32_t thread, uint32_t u_axis, uint32_t U, uint32_t u_shift, uint32_t V, uint32_t v_shift, uint32_t tu, uint32_t tv,
                                             uint32_t &vx, uint32_t &vy, uint32_t &lane_u, uint32_t &lane_v)
{
	if (u_axis == 0) { lane_u = thread & (U - 1); lane_v = thread >> u_shift; }
	else             { lane_v = thread & (V - 1); lane_u = thread >> v_shift; }
	const uint32_t gu = tu * U + lane_u, gv = tv * V + lane_v;
	vx = u_axis == 0 ? gu : gv; vy = u_axis == 0 ? gv : gu;
}

/* the voxel's value, coherency weighted where asked, into plane zl of the shard's output */
template <bool CW, typename Value>
__device__ __forceinline__ void rca_store_voxel(const BfDasArgs &p, uint32_t zl, uint32_t x, uint32_t y, Value coherent, float incoherent)
{
	uint64_t out_index = (uint64_t)p.size[0] * p.size[1] * zl + (uint64_t)p.size[0] * y + x;
	reinterpret_cast<Value *>(p.out)[out_index] = coherency_weighted<CW>(coherent, incoherent);
}

/* ---- host: grid from the tile count (a multiple of 8: one run of tiles per XCD), the dynamic LDS limit, the launch */
template <typename Kernel>
static hipError_t rca_launch_tiles(Kernel kernel, uint32_t total, uint32_t threads, const BfDasArgs *a, const BfSeparableArgs *q, hipStream_t s)
{
	const uint32_t grid = ((total + 7u) / 8u) * 8u;
	hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)q->lds_bytes);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), q->lds_bytes, s, *a, *q);
	return hipGetLastError();
}

/* f(VS, WS) as integral constants for the tile's extent along the transmit axis and the window length (log2) of q */
template <typename F>
static hipError_t staged_for_shape(const BfSeparableArgs *q, F &&f)
{
	using std::integral_constant;
	switch ((q->v_shift << 4) | q->window_shift) {
	case (4 << 4) | 5: return f(integral_constant<int, 4>{}, integral_constant<int, 5>{});
	case (5 << 4) | 5: return f(integral_constant<int, 5>{}, integral_constant<int, 5>{});
	case (6 << 4) | 5: return f(integral_constant<int, 6>{}, integral_constant<int, 5>{});
	case (4 << 4) | 6: return f(integral_constant<int, 4>{}, integral_constant<int, 6>{});
	case (5 << 4) | 6: return f(integral_constant<int, 5>{}, integral_constant<int, 6>{});
	case (6 << 4) | 6: return f(integral_constant<int, 6>{}, integral_constant<int, 6>{});
	}
	return hipErrorInvalidValue;
}

/* f(NL) for the passes a thread stages per channel (whole windows per wave): ceil(A4 * W / threads), 1 to 4 */
static inline uint32_t staged_passes(const BfDasArgs *a, const BfSeparableArgs *q, int window_shift)
{
	const uint32_t A4 = ((uint32_t)a->acquisition_count + 3u) & ~3u;
	return ((A4 << window_shift) + q->threads - 1) / q->threads;
}
template <typename F>
static hipError_t staged_for_passes(uint32_t passes, F &&f)
{
	switch (passes) {
	case 1: return f(std::integral_constant<int, 1>{});
	case 2: return f(std::integral_constant<int, 2>{});
	case 3: return f(std::integral_constant<int, 3>{});
	case 4: return f(std::integral_constant<int, 4>{});
	}
	return hipErrorInvalidValue;
}

#endif
