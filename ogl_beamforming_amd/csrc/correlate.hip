/* correlate.hip -- the shift correlation of the K newest frames of the frame ring against one of them
 * (beamformer_hip_correlate_last_frames): for every box b, frame k and integer shift s of the window,
 *     C = sum conj(ref[v]) f_k[v + s],   sum |ref[v]|^2,   sum |f_k[v + s]|^2,   the number of terms,
 * over the voxels v of the box with v + s inside the FRAME and both voxels finite.  include/ogl_beamformer_hip.h has the definition
 * for callers; tests/motion_ref.py restates it in numpy.
 *
 * ARITHMETIC.  The Gram matrix's (ensemble.hip): every float widened to double, the products of two widened floats exact, so
 * rj * rk + ij * ik, rj * ik - ij * rk and r * r + i * i are ONE rounding each, written as an fma; adding a term to its running sum
 * is one more.  Real frames take i = 0 (the instantiation without the imaginary arithmetic stores im = +0).
 *
 * Two launches, no atomics:
 *   partial  grid x the chunk -- a run of bf_correlate_chunk_tiles tiles of the box, in flat tile order --, grid y the frame k, grid z
 *            the box.  A tile is bf_correlate_tile's: at most 1024 voxels, at most 4096 with its halo of S voxels either side; tile and
 *            chunking are functions of the box and the window alone.  Per tile the block stages, once for all T shifts,
 *              tile[n]   the reference's voxel n of the tile (flat in the tile, x fastest) as {re, im, the voxel's offset in the halo
 *                        array, valid}: 16 bytes, read by ONE ds_read_b128; valid = inside the box and finite, else re = im = 0;
 *              halo[e]   frame k's voxels of the tile plus its halo (8 bytes each) and ok[e], a byte: inside the frame and finite --
 *                        a voxel that is not is staged as +0, so that its products and its square add nothing, and the inner loop
 *                        tests no float: ok[e] gates energy_reference and counts the terms.
 *            THREADS OWN SHIFTS, each with its five accumulators.  T <= 255: G = floor(256 / T) groups of T threads; thread t is shift
 *            s = t % T of group g = t / T (threads from G T on idle: 4 of 256 at T = 9, 6 at T = 25, 13 at T = 81; a window of 129
 *            to 255 shifts is one group and leaves 256 - T threads idle, as the last batch of a larger window does -- 1089 shifts
 *            fill 85 % of five batches), and group g takes the tile's voxels n = g, g + G, ...: within a wave the groups read consecutive
 *            tile entries (distinct banks), a group's threads the same one (a broadcast), and the halo reads of consecutive sx are
 *            consecutive addresses.  T > 256: one group, thread t owns the shifts t, t + 256, ... (at most 5: the accumulators of
 *            all of them live in registers across the tiles of the chunk; the batch loop is unrolled, a batch past T is skipped by
 *            a uniform test).  A reference voxel that is not valid is skipped whole.  After the chunk's last tile the groups'
 *            sums of a shift are added in ascending g through LDS (the halo array's memory), and one entry a shift is stored.
 *   fold     a thread an entry (box, frame, shift) of the table sums its chunks' partials in chunk order; no term: 40 zero bytes.
 * The order of every addition is fixed by the box and the window: the bytes of an entry do not depend on K, on the other frames, on
 * the other boxes or on the call being repeated. */
#include <hip/hip_runtime.h>
#include "bf_kernels.h"

namespace {

typedef float corr_f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t corr_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool is_finite(float a) { return (__float_as_uint(a) & 0x7F800000u) != 0x7F800000u; }

template <bool CPLX>
__device__ __forceinline__ corr_f32x2 voxel_at(const char *frame, uint64_t i)
{
	if (CPLX) return ((const corr_f32x2 *)frame)[i];
	corr_f32x2 r; r.x = ((const float *)frame)[i]; r.y = 0.0f;
	return r;
}

struct Sums { double re, im, er, ef; uint32_t terms; };

} // namespace

template <bool CPLX>
__global__ __launch_bounds__(BF_CORRELATE_THREADS) void correlate_partial_kernel(const char *__restrict__ ring, const uint64_t *__restrict__ offsets,
                                                                                 const BfCorrelateRow *__restrict__ rows, BfCorrelateArgs a,
                                                                                 BfCorrelateEntry *__restrict__ partials)
{
	#pragma clang fp contract(off)
	__shared__ corr_f32x2 halo[BF_CORRELATE_HALO_VOXELS];
	__shared__ corr_u32x4 tile[BF_CORRELATE_TILE_VOXELS];
	__shared__ uint8_t    ok[BF_CORRELATE_HALO_VOXELS];

	const BfCorrelateRow &row = rows[blockIdx.z];
	const uint32_t chunk = blockIdx.x;
	if (chunk >= row.chunks) return;                          /* (the whole block: grid x is the most chunks any box has) */
	const uint32_t k = blockIdx.y, tid = threadIdx.x;
	const char *reference = ring + offsets[a.reference], *frame = ring + offsets[k];

	const uint32_t cx = row.count[0], cy = row.count[1], cz = row.count[2];
	const uint32_t tx = row.tile[0], ty = row.tile[1];
	const uint32_t hx = row.halo[0], hy = row.halo[1];
	const uint32_t tile_voxels = row.tile_voxels, halo_voxels = row.halo_voxels;
	const uint32_t px = a.points[0], py = a.points[1], pz = a.points[2];

	/* the thread's group and its shifts' offsets in the halo array */
	const uint32_t T = a.shifts, G = a.groups;
	const uint32_t g = tid / T, s0 = tid - g * T;             /* (T > 256: g = 0, s0 = tid) */
	uint32_t base[BF_CORRELATE_MAX_BATCHES];
	bool     live[BF_CORRELATE_MAX_BATCHES];
	#pragma unroll
	for (uint32_t b = 0; b < BF_CORRELATE_MAX_BATCHES; b++) {
		const uint32_t s = s0 + b * BF_CORRELATE_THREADS;
		live[b] = b < a.batches && g < G && s < T;
		const uint32_t rest = s / a.window[0], sx = s - rest * a.window[0], sz = rest / a.window[1], sy = rest - sz * a.window[1];
		base[b] = live[b] ? (sz * hy + sy) * hx + sx : 0u;
	}
	Sums sum[BF_CORRELATE_MAX_BATCHES];
	#pragma unroll
	for (uint32_t b = 0; b < BF_CORRELATE_MAX_BATCHES; b++) { sum[b].re = 0.0; sum[b].im = 0.0; sum[b].er = 0.0; sum[b].ef = 0.0; sum[b].terms = 0; }

	const uint32_t tiles = row.tiles[0] * row.tiles[1] * row.tiles[2];
	const uint32_t tile_first = chunk * row.chunk_tiles;
	const uint32_t tile_end = tile_first + row.chunk_tiles < tiles ? tile_first + row.chunk_tiles : tiles;
	for (uint32_t t = tile_first; t < tile_end; t++) {
		const uint32_t trest = t / row.tiles[0], tix = t - trest * row.tiles[0], tiz = trest / row.tiles[1], tiy = trest - tiz * row.tiles[1];
		const uint32_t ox = tix * tx, oy = tiy * ty, oz = tiz * row.tile[2];     /* the tile's first voxel in the box */

		/* frame k: the tile and its halo; entry (0, 0, 0) is the frame's voxel first + o - S */
		for (uint32_t e = tid; e < halo_voxels; e += BF_CORRELATE_THREADS) {
			const uint32_t rest = e / hx, x = e - rest * hx, z = rest / hy, y = rest - z * hy;
			const int64_t fx = (int64_t)row.first[0] + ox + x - a.max_shift[0], fy = (int64_t)row.first[1] + oy + y - a.max_shift[1],
			              fz = (int64_t)row.first[2] + oz + z - a.max_shift[2];
			corr_f32x2 c; c.x = 0.0f; c.y = 0.0f;
			bool good = fx >= 0 && fx < (int64_t)px && fy >= 0 && fy < (int64_t)py && fz >= 0 && fz < (int64_t)pz;
			if (good) {
				c = voxel_at<CPLX>(frame, ((uint64_t)fz * py + (uint64_t)fy) * px + (uint64_t)fx);
				good = is_finite(c.x) && is_finite(c.y);
				if (!good) { c.x = 0.0f; c.y = 0.0f; }
			}
			halo[e] = c;
			ok[e] = good ? 1u : 0u;
		}
		/* the reference: the tile's voxels, those past the box's end not valid */
		for (uint32_t n = tid; n < tile_voxels; n += BF_CORRELATE_THREADS) {
			const uint32_t rest = n / tx, x = n - rest * tx, z = rest / ty, y = rest - z * ty;
			corr_f32x2 c; c.x = 0.0f; c.y = 0.0f;
			bool good = ox + x < cx && oy + y < cy && oz + z < cz;
			if (good) {
				c = voxel_at<CPLX>(reference, ((uint64_t)(row.first[2] + oz + z) * py + (row.first[1] + oy + y)) * px + (row.first[0] + ox + x));
				good = is_finite(c.x) && is_finite(c.y);
				if (!good) { c.x = 0.0f; c.y = 0.0f; }
			}
			corr_u32x4 q;
			q.x = __float_as_uint(c.x); q.y = __float_as_uint(c.y); q.z = (z * hy + y) * hx + x; q.w = good ? 1u : 0u;
			tile[n] = q;
		}
		__syncthreads();
		#pragma unroll
		for (uint32_t b = 0; b < BF_CORRELATE_MAX_BATCHES; b++) {
			if (!live[b]) continue;
			Sums acc = sum[b];
			for (uint32_t n = g; n < tile_voxels; n += G) {
				const corr_u32x4 q = tile[n];
				if (!q.w) continue;
				const uint32_t at = base[b] + q.z;                /* (at most halo_voxels - 1: the tile's last voxel under the last shift) */
				const corr_f32x2 f = halo[at];
				const bool fine = ok[at] != 0;
				const double rj = (double)__uint_as_float(q.x), rk = (double)f.x;
				if (CPLX) {
					const double ij = (double)__uint_as_float(q.y), ik = (double)f.y;
					acc.re = acc.re + __builtin_fma(ij, ik, rj * rk);
					acc.im = acc.im + __builtin_fma(-ij, rk, rj * ik);
					acc.ef = acc.ef + __builtin_fma(ik, ik, rk * rk);
					acc.er = acc.er + (fine ? __builtin_fma(ij, ij, rj * rj) : 0.0);
				} else {
					acc.re = acc.re + rj * rk;
					acc.ef = acc.ef + rk * rk;
					acc.er = acc.er + (fine ? rj * rj : 0.0);
				}
				acc.terms += fine ? 1u : 0u;
			}
			sum[b] = acc;
		}
		__syncthreads();
	}

	BfCorrelateEntry *out = partials + row.partial_first + ((uint64_t)chunk * a.frames + k) * T;
	if (G > 1u) {
		/* the groups' sums of a shift, added in ascending g: [g T + s] is thread g T + s's own slot */
		double   *part  = (double *)halo;                         /* 4 x 256 doubles, then 256 counts: 9 KiB of the halo array's 32 */
		uint32_t *count = (uint32_t *)(part + 4u * BF_CORRELATE_THREADS);
		part[tid] = sum[0].re; part[BF_CORRELATE_THREADS + tid] = sum[0].im;
		part[2u * BF_CORRELATE_THREADS + tid] = sum[0].er; part[3u * BF_CORRELATE_THREADS + tid] = sum[0].ef;
		count[tid] = sum[0].terms;
		__syncthreads();
		if (tid >= T) return;
		Sums total; total.re = 0.0; total.im = 0.0; total.er = 0.0; total.ef = 0.0; total.terms = 0;
		for (uint32_t group = 0; group < G; group++) {
			const uint32_t at = group * T + tid;
			total.re = total.re + part[at]; total.im = total.im + part[BF_CORRELATE_THREADS + at];
			total.er = total.er + part[2u * BF_CORRELATE_THREADS + at]; total.ef = total.ef + part[3u * BF_CORRELATE_THREADS + at];
			total.terms += count[at];
		}
		BfCorrelateEntry e; e.re = total.re; e.im = CPLX ? total.im : 0.0; e.energy_reference = total.er; e.energy_frame = total.ef; e.terms = total.terms;
		out[tid] = e;
		return;
	}
	#pragma unroll
	for (uint32_t b = 0; b < BF_CORRELATE_MAX_BATCHES; b++) {
		if (!live[b]) continue;
		BfCorrelateEntry e; e.re = sum[b].re; e.im = CPLX ? sum[b].im : 0.0; e.energy_reference = sum[b].er; e.energy_frame = sum[b].ef; e.terms = sum[b].terms;
		out[s0 + b * BF_CORRELATE_THREADS] = e;
	}
}

__global__ __launch_bounds__(256) void correlate_fold_kernel(const BfCorrelateRow *__restrict__ rows, BfCorrelateArgs a,
                                                             const BfCorrelateEntry *__restrict__ partials, BfCorrelateEntry *__restrict__ table)
{
	#pragma clang fp contract(off)
	const uint32_t per_region = a.frames * a.shifts;              /* (regions x frames x shifts <= 2^20) */
	const uint32_t entry = blockIdx.x * 256u + threadIdx.x;
	if (entry >= a.regions * per_region) return;
	const uint32_t region = entry / per_region;
	const BfCorrelateRow &row = rows[region];
	const BfCorrelateEntry *p = partials + row.partial_first + (entry - region * per_region);
	BfCorrelateEntry total; total.re = 0.0; total.im = 0.0; total.energy_reference = 0.0; total.energy_frame = 0.0; total.terms = 0;
	for (uint32_t chunk = 0; chunk < row.chunks; chunk++, p += per_region) {
		const BfCorrelateEntry t = *p;
		total.re = total.re + t.re; total.im = total.im + t.im;
		total.energy_reference = total.energy_reference + t.energy_reference; total.energy_frame = total.energy_frame + t.energy_frame;
		total.terms += t.terms;
	}
	if (!total.terms) { total.re = 0.0; total.im = 0.0; total.energy_reference = 0.0; total.energy_frame = 0.0; }
	table[entry] = total;
}

/* Every table is device memory.  Every box lies inside the frames and every frame inside the ring: the caller's business (frame_ops.cpp:
 * correlate_last_frames); what is checked here is that the rows' geometry fits the kernel's LDS arrays -- the caller reads the rows
 * back from where it made them, the launcher cannot. */
extern "C" hipError_t bf_launch_correlate(const void *ring, const uint64_t *offsets, const BfCorrelateRow *rows, const BfCorrelateArgs *a,
                                          BfCorrelateEntry *partials, BfCorrelateEntry *table, hipStream_t s)
{
	static_assert(sizeof(BfCorrelateEntry) == 40 && sizeof(BfCorrelateRow) % 8 == 0, "records without padding");
	if (!ring || !offsets || !rows || !a || !partials || !table || a->frames == 0 || a->frames > BF_ENSEMBLE_MAX_FRAMES || a->reference >= a->frames ||
	    a->regions == 0 || a->regions > 65535u || a->shifts == 0 || a->shifts > BF_CORRELATE_MAX_SHIFTS || a->max_chunks == 0 ||
	    a->groups != bf_correlate_groups(a->shifts) || a->batches != (a->shifts + BF_CORRELATE_THREADS - 1u) / BF_CORRELATE_THREADS ||
	    (uint64_t)a->regions * a->frames * a->shifts > (1ull << 20))
		return hipErrorInvalidValue;
	for (int k = 0; k < 3; k++)
		if (a->max_shift[k] > BF_CORRELATE_MAX_SHIFT || a->window[k] != 2u * a->max_shift[k] + 1u) return hipErrorInvalidValue;
	if (a->shifts != a->window[0] * a->window[1] * a->window[2]) return hipErrorInvalidValue;
	if (a->cplx) hipLaunchKernelGGL(correlate_partial_kernel<true>, dim3(a->max_chunks, a->frames, a->regions), dim3(BF_CORRELATE_THREADS), 0, s,
	                                (const char *)ring, offsets, rows, *a, partials);
	else         hipLaunchKernelGGL(correlate_partial_kernel<false>, dim3(a->max_chunks, a->frames, a->regions), dim3(BF_CORRELATE_THREADS), 0, s,
	                                (const char *)ring, offsets, rows, *a, partials);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	const uint32_t entries = a->regions * a->frames * a->shifts;
	hipLaunchKernelGGL(correlate_fold_kernel, dim3((entries + 255u) / 256u), dim3(256), 0, s, rows, *a, (const BfCorrelateEntry *)partials, table);
	return hipGetLastError();
}
