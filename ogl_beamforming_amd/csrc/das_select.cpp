/* das_select.cpp -- which DAS kernel a frame runs, and why (das_select.h).  Host arithmetic only.
 *
 * The rules, in the order decide_das tries them -- one function each; the first that takes the frame ends the ladder:
 *   rule_zero       (no kernel)        a family or interpolation mode the shader leaves at zero: the frame is cleared
 *   rule_separable  das_separable.hip  gather: row-column frames whose receive and transmit delays separate over the tile axes (plan_separable)
 *                   das_staged*.hip    staged: ... and whose delay spread provably fits an LDS window (plan_staged), from kStagedMinTransmits;
 *                                      its transmit tables global under the table cap, else in LDS, else back to the gather kernel
 *   rule_hercules   das_hercules.hip   HERCULES family on array-aligned grids, volumes and view planes (plan_hercules)
 *   rule_tile       das_tile.hip       cubic IQ frames the factored kernel would run, on grids fine enough that a 64 x 16 tile fits a staged window
 *   rule_factored   das_factored.hip   any frame whose index is a receive term plus a transmit term (factored_applies)
 *   rule_general    das.hip            every family; asked for by path 1; the fallback
 * fill_das_args fills the arguments in front of them and chooses nothing.  A rule that declines writes why[] of its own path and of no
 * other; a rule that takes the frame also speaks for the rules behind it, which are not tried.  A new kernel is a new rule_* at its
 * place in the ladder: one line in decide_das and one here (tests/select_digest.cpp shows which decisions it moves).
 */
#include "das_select.h"
#include "host_math.h"
#include "../../include/ogl_beamformer_lib.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace bf {

const char *das_path_name(int path)
{
	static const char *names[] = {"general kernel", "separable-delay gather kernel", "separable-delay LDS-staged kernel", "per-voxel factored kernel",
	                              "HERCULES aligned-grid kernel", "per-voxel factored kernel with block-wide LDS staging",
	                              "?", "none: the frame is cleared"};
	return path >= 0 && path <= 7 ? names[path] : "?";
}

const char *das_kernel_name(int path)
{
	static const char *names[] = {"das_kernel", "das_rca_separable_kernel", "das_rca_staged_kernel", "das_factored_kernel",
	                              "das_hercules_kernel", "das_tile_kernel", "?", "(none)"};
	return path >= 0 && path <= 7 ? names[path] : "?";
}

/* ---------------------------------------------------------------- hooks */

static Hooks g_hooks;
static const char *const g_hook_names[] = {"STAGED_SHAPE", "STAGED_CHECKED", "STAGED_NOUNIFORM", "STAGED_TABLE_CAP", "DEBUG", "SCRATCH_POISON", nullptr};
const char *const *hook_names() { return g_hook_names; }

static bool apply_hook(Hooks &h, const char *name, const char *value)
{
	const bool on = value && value[0];
	if (!std::strcmp(name, "STAGED_SHAPE")) {
		unsigned u = 0, v = 0, w = 0;
		h.staged_shape_set = on && std::sscanf(value, "%u,%u,%u", &u, &v, &w) == 3;
		h.staged_shape[0] = (int)u; h.staged_shape[1] = (int)v; h.staged_shape[2] = (int)w;
	}
	else if (!std::strcmp(name, "STAGED_CHECKED"))   h.staged_checked = on;
	else if (!std::strcmp(name, "STAGED_NOUNIFORM")) h.staged_nouniform = on;
	else if (!std::strcmp(name, "STAGED_TABLE_CAP")) h.staged_table_cap = on ? std::strtoull(value, nullptr, 0) : (2ull << 30);
	else if (!std::strcmp(name, "DEBUG"))            h.debug = on;
	else if (!std::strcmp(name, "SCRATCH_POISON"))   h.scratch_poison = on;
	else return false;
	return true;
}

Hooks &hooks() { return g_hooks; }

bool set_hook(const char *name, const char *value)
{
	Hooks &h = hooks();
	if (!name || !apply_hook(h, name, value)) return false;
	h.version++;
	return true;
}

/* ---------------------------------------------------------------- geometry rules */

static uint32_t ceil_log2(uint32_t v) { uint32_t s = 0; while ((1u << s) < v) s++; return s; }
/* blocks of 2^shift voxels (tiles, columns) that cover `extent` voxels of an axis */
static uint32_t blocks_at(uint32_t extent, uint32_t shift) { return (extent + (1u << shift) - 1) >> shift; }

/* Shape of the 2^tile_log2-voxel block of the DAS launch.  The axis along which the transducer-space
 * depth changes fastest gets extent 1: sample indices move ~2 samples per voxel along depth
 * but only a fraction of a sample per voxel laterally, so a depth-flat tile keeps the 64 lanes
 * of a wave within a few cache lines of every (channel, transmit) row. */
static int choose_tile(const float *voxel_to_xdc, const uint32_t size[3], uint32_t zcount, uint32_t shift[3], uint32_t tile_log2 = 8)
{
	uint32_t extent[3] = {size[0], size[1], zcount};
	uint32_t full[3]   = {size[0], size[1], size[2]};
	int depth = -1; float best = -1;
	for (int i = 0; i < 3; i++) {
		if (extent[i] <= 1) continue;
		float step = std::fabs(voxel_to_xdc[4 * i + 2]) / (float)(full[i] > 1 ? full[i] - 1 : 1);
		if (step > best) { best = step; depth = i; }
	}
	uint32_t cap[3], left = tile_log2;
	for (int i = 0; i < 3; i++) { cap[i] = ceil_log2(extent[i]); shift[i] = 0; }
	int lateral[2], nl = 0;
	for (int i = 0; i < 3; i++) if (i != depth && extent[i] > 1) lateral[nl++] = i;
	uint32_t first = nl == 2 ? tile_log2 / 2 : tile_log2;
	for (int k = 0; k < nl; k++) {
		uint32_t give = cap[lateral[k]] < first ? cap[lateral[k]] : first;
		if (give > left) give = left;
		shift[lateral[k]] = give; left -= give;
	}
	for (int k = 0; k < nl && left; k++) {
		uint32_t room = cap[lateral[k]] - shift[lateral[k]];
		uint32_t give = room < left ? room : left;
		shift[lateral[k]] += give; left -= give;
	}
	if (depth >= 0 && left) {
		uint32_t give = cap[depth] < left ? cap[depth] : left;
		shift[depth] = give; left -= give;
	}
	shift[0] += left;   /* fewer voxels in total than the tile: idle lanes */
	return depth;
}

/* tile walk of the kernels that deal tiles to the XCDs in contiguous runs: the depth axis runs fastest, so that a run is a
 * lateral column at every depth (neighbouring RF windows AND the same work on every XCD: the f-number test culls shallow
 * voxels).  Volumes: depth = voxel z (1); the reference's view planes (math.c:844-885) put it on voxel y (2). */
static uint32_t tile_walk(int depth_axis, uint32_t zcount, uint32_t tile_rows, uint32_t &band_rows)
{
	band_rows = 1;
	if (depth_axis != 1) return 1u;
	if (zcount != 1) return 2u;
	/* view plane: ~32 bands, four per XCD (bf_plane_walk) */
	band_rows = tile_rows / 32u ? tile_rows / 32u : 1u;
	return 3u;
}

/* Samples of delay one voxel step along x (the lane axis of the per-voxel kernels) can move a sample index: the physical
 * length of the step times fs / c.  >= 1: a COARSE grid -- neighbouring lanes read different samples of an RF row. */
static float lane_step_samples(const float *voxel_to_xdc, const BfDasArgs &a)
{
	const float n = (float)(a.size[0] > 1 ? a.size[0] - 1 : 1);
	const float dx = voxel_to_xdc[0] / n, dy = voxel_to_xdc[1] / n, dz = voxel_to_xdc[2] / n;
	return std::sqrt(dx * dx + dy * dy + dz * dz) * a.sampling_frequency * a.inv_speed_of_sound;
}

/* das_tile.hip: an upper bound of (largest - smallest receive index) + (largest - smallest transmit index) over a tile of
 * 2^shift voxels, in samples -- what a staged window has to hold.  Per voxel axis, from the derivatives of the two distances:
 * the receive distance sqrt(lateral^2 + z^2) moves by at most sin(theta) per unit of lateral step, and the f-number test
 * (|lateral| f / z < 1/2, das.glsl:205-207) keeps sin(theta) under 1 / sqrt(1 + 4 f^2), and by at most 1 per unit of depth; a plane
 * wave's by |sin a| laterally and by at most 1 in depth; a focused or diverging wave's, and a FORCES transmit element's, by at
 * most the length of the step.  (The kernel measures the real spread per block and chunk: the estimate only decides whether the
 * block-staged kernel is worth launching.) */
static float tile_spread_estimate(const BfDasArgs &a, const std::vector<BfTransmit> &tx, const float *voxel_to_xdc, const float *voxel_to_world,
                                  const uint32_t shift[3])
{
	const float sin_rx = 1.0f / std::sqrt(1.0f + 4.0f * a.f_number * a.f_number);
	const float samples_per_metre = a.sampling_frequency * a.inv_speed_of_sound;
	float spread = 2.0f;                                                   /* the two floors */
	for (int k = 0; k < 3; k++) {
		const float n = (float)(a.size[k] > 1 ? a.size[k] - 1 : 1);
		const float xs[3] = {voxel_to_xdc[4 * k + 0] / n, voxel_to_xdc[4 * k + 1] / n, voxel_to_xdc[4 * k + 2] / n};
		const float ws[3] = {voxel_to_world[4 * k + 0] / n, voxel_to_world[4 * k + 1] / n, voxel_to_world[4 * k + 2] / n};
		float receive, transmit = 0.f;
		if (a.family == BF_DAS_RCA) {
			const bool rx_rows = !tx.empty() && (tx[0].flags & BF_RX_ROWS);
			receive = sin_rx * std::fabs(rx_rows ? xs[1] : xs[0]) + std::fabs(xs[2]);
			for (const BfTransmit &t : tx) {
				if (t.flags & BF_TX_NONE) continue;
				const float px = (t.flags & BF_TX_ROWS) ? ws[1] : ws[0];
				const float step = (t.flags & BF_TX_PLANE) ? std::fabs(px * t.sin_a) + std::fabs(ws[2] * t.cos_a) : std::sqrt(px * px + ws[2] * ws[2]);
				transmit = step > transmit ? step : transmit;
			}
		} else {
			receive  = sin_rx * std::fabs(xs[0]) + std::fabs(xs[2]);
			transmit = std::sqrt(xs[0] * xs[0] + xs[1] * xs[1] + xs[2] * xs[2]);
		}
		spread += (receive + transmit) * samples_per_metre * (float)((1u << shift[k]) - 1u);
	}
	return spread;
}

/* das_tile.hip: the spread the kernel itself would measure -- (floor max R_c - floor min R_c over the voxels inside channel c's aperture) +
 * max over the transmits of (floor max T_a - floor min T_a) -- evaluated in double precision over a 5 x 5 x 2 lattice of voxels (the
 * corners among them) of up to 27 tiles: first, middle and last along every axis, where the extremes of an image lie.  Sharper than
 * tile_spread_estimate's derivative bound (config 2: 24 against 27.9), not an upper bound (lattice, sampled tiles): the kernel still
 * decides per block and chunk, and a chunk that does not fit runs its gather loop.  Returns the largest such sum (+ 1 for the lattice). */
static float tile_spread_sampled(const BfDasArgs &a, const std::vector<BfTransmit> &tx, const ParameterBlock &pb, const float *voxel_to_world,
                                 const uint32_t ext[3], const uint32_t shift[3], uint32_t zfirst)
{
	if (tx.empty() && a.family == BF_DAS_RCA) return 0.f;
	const double fs_over_c = (double)a.sampling_frequency * (double)a.inv_speed_of_sound;
	const int C = a.channel_count, A = a.acquisition_count;
	const int first_transmit = a.family == BF_DAS_RCA ? 0 : (a.sparse != 0);
	const bool rx_rows = a.family == BF_DAS_RCA && (tx[0].flags & BF_RX_ROWS);
	auto point = [](const float *m, double x, double y, double z, double o[3]) {
		for (int r = 0; r < 3; r++) o[r] = m[r] * x + m[4 + r] * y + m[8 + r] * z + m[12 + r];
	};
	uint32_t tiles[3][3], tile_count[3];
	for (int k = 0; k < 3; k++) {
		const uint32_t n = blocks_at(ext[k], shift[k]);
		tiles[k][0] = 0; tiles[k][1] = n / 2; tiles[k][2] = n - 1;
		tile_count[k] = n >= 3 ? 3 : n == 2 ? 2 : 1;
		if (n == 2) tiles[k][1] = 1;
	}
	double worst = 0;
	std::vector<double> rlo((size_t)C), rhi((size_t)C), tlo((size_t)A), thi((size_t)A);
	for (uint32_t iz = 0; iz < tile_count[2]; iz++) for (uint32_t iy = 0; iy < tile_count[1]; iy++) for (uint32_t ix = 0; ix < tile_count[0]; ix++) {
		const uint32_t t0[3] = {tiles[0][ix] << shift[0], tiles[1][iy] << shift[1], tiles[2][iz] << shift[2]};
		std::fill(rlo.begin(), rlo.end(), 1e30); std::fill(rhi.begin(), rhi.end(), -1e30);
		std::fill(tlo.begin(), tlo.end(), 1e30); std::fill(thi.begin(), thi.end(), -1e30);
		for (int sz = 0; sz < 2; sz++) for (int sy = 0; sy < 5; sy++) for (int sx = 0; sx < 5; sx++) {
			uint32_t v[3];
			const int step[3] = {sx, sy, sz * 4};
			for (int k = 0; k < 3; k++) {
				const uint32_t span = (1u << shift[k]) - 1u;
				v[k] = t0[k] + (uint32_t)((uint64_t)span * (uint32_t)step[k] / 4u);
				if (v[k] >= ext[k]) v[k] = ext[k] - 1;                       /* ragged tiles: threads outside the grid repeat its last voxel */
			}
			const double px = (double)v[0] / std::fmax(1.0, (double)a.size[0] - 1.0), py = (double)v[1] / std::fmax(1.0, (double)a.size[1] - 1.0);
			const double pz = (double)(v[2] + zfirst) / std::fmax(1.0, (double)a.size[2] - 1.0);
			double w[3], x[3];
			point(voxel_to_world, px, py, pz, w);
			if (a.family == BF_DAS_RCA) point(a.xdc_transform, w[0], w[1], w[2], x); else { x[0] = w[0]; x[1] = w[1]; x[2] = w[2]; }
			const double lateral = rx_rows ? x[1] : x[0], pitch = rx_rows ? a.pitch[1] : a.pitch[0];
			for (int c = 0; c < C; c++) {
				const double dx = lateral - c * pitch;
				if (!(std::fabs(dx * a.f_number / std::fabs(x[2])) < 0.5)) continue;
				const double r = std::sqrt(dx * dx + x[2] * x[2]) * fs_over_c;
				rlo[(size_t)c] = std::fmin(rlo[(size_t)c], r); rhi[(size_t)c] = std::fmax(rhi[(size_t)c], r);
			}
			for (int t = first_transmit; t < A; t++) {
				double d = 0;
				if (a.family == BF_DAS_RCA) {
					const BfTransmit &q = tx[(size_t)t];
					if (!(q.flags & BF_TX_NONE)) {
						const double p = (q.flags & BF_TX_ROWS) ? w[1] : w[0];
						d = (q.flags & BF_TX_PLANE) ? p * q.sin_a + w[2] * q.cos_a : std::sqrt((p - q.focus_x) * (p - q.focus_x) + (w[2] - q.focus_z) * (w[2] - q.focus_z));
					}
				} else {
					const double element = a.sparse ? (double)pb.sparse_elements[t - first_transmit] : (double)t;
					const double dy = x[1] - a.pitch[1] * C * 0.5, tdx = x[0] - a.pitch[0] * element;
					d = std::sqrt(dy * dy + x[2] * x[2] + tdx * tdx);
				}
				d *= fs_over_c;
				tlo[(size_t)t] = std::fmin(tlo[(size_t)t], d); thi[(size_t)t] = std::fmax(thi[(size_t)t], d);
			}
		}
		double ts = 0, rs = 0;
		for (int t = first_transmit; t < A; t++) ts = std::fmax(ts, std::floor(thi[(size_t)t]) - std::floor(tlo[(size_t)t]));
		for (int c = 0; c < C; c++) if (rlo[(size_t)c] <= rhi[(size_t)c]) rs = std::fmax(rs, std::floor(rhi[(size_t)c]) - std::floor(rlo[(size_t)c]));
		worst = std::fmax(worst, rs + ts);
	}
	return (float)(worst + 1.0);
}

/* Can this RCA frame use the separable-delay fast path (das_separable.hip)?  Needs one
 * receive and one transmit orientation for all transmits, on different transducer axes, a
 * volume whose z axis alone carries depth, and voxel x / y axes that each move only one of
 * the two lateral coordinates -- every coefficient that must vanish has to be an exact
 * zero product, so that the tables reproduce the general kernel's per-voxel arithmetic. */
static bool plan_separable(const BfDasArgs &a, const std::vector<BfTransmit> &tx, const float *xdc, const float *vox,
                           uint32_t zcount, BfSeparableArgs &q)
{
	if (a.family != BF_DAS_RCA || tx.empty()) return false;
	const uint32_t orient = BF_TX_ROWS | BF_RX_ROWS | BF_TX_NONE;
	for (const BfTransmit &t : tx) if ((t.flags & orient) != (tx[0].flags & orient)) return false;
	const bool tx_none = (tx[0].flags & BF_TX_NONE) != 0;
	const int  r = (tx[0].flags & BF_RX_ROWS) ? 1 : 0;      /* transducer coordinate the receive aperture uses */
	const int  w = (tx[0].flags & BF_TX_ROWS) ? 1 : 0;      /* world coordinate the transmit uses */
	auto W = [&](int row, int col) { return vox[4 * col + row]; };
	auto X = [&](int row, int col) { return xdc[4 * col + row]; };
	/* transducer coordinate `row` must not move with voxel axis `col` */
	auto xdc_fixed = [&](int row, int col) {
		for (int k = 0; k < 3; k++) if (X(row, k) != 0.f && W(k, col) != 0.f) return false;
		return true;
	};
	if (a.size[0] < 2 || a.size[1] < 2) return false;
	for (int col = 0; col < 2; col++) {
		if (!xdc_fixed(2, col)) return false;                 /* transducer depth: voxel z only */
		if (!tx_none && W(2, col) != 0.f) return false;       /* world depth: voxel z only */
	}
	int u_axis = -1;
	for (int u = 0; u < 2 && u_axis < 0; u++) {
		int v = 1 - u;
		if (!xdc_fixed(r, v)) continue;                       /* receive lateral: not along v */
		if (!tx_none && W(w, u) != 0.f) continue;             /* transmit lateral: not along u */
		u_axis = u;
	}
	if (u_axis < 0) return false;

	/* Tile (U along the receive axis, V along the transmit axis), block size and the number of
	 * channels per receive-table chunk: maximise resident waves per CU (LDS: 160 KB per CU, 32
	 * waves per CU), then prefer big chunks (fewer rebuilds) and square-ish tiles. */
	const uint32_t C = (uint32_t)a.channel_count, A = (uint32_t)a.acquisition_count;
	const uint32_t lds_cu = 160u * 1024u;
	uint32_t best_waves = 0, best_score = 0;
	for (uint32_t threads_shift = 10; threads_shift >= 8; threads_shift--) {
		for (uint32_t us = 2; us + 2 <= threads_shift; us++) {
			uint32_t vs = threads_shift - us;
			if ((u_axis == 0 ? us : vs) < 4) continue;        /* >= 16 lanes of a wave along x */
			for (uint32_t chunk = 16; chunk <= 256; chunk *= 2) {
				uint32_t cc = chunk < C ? chunk : C;
				uint64_t lds = 16ull * (((uint64_t)cc << us) + ((uint64_t)A << vs));
				if (lds > lds_cu) continue;
				uint32_t blocks = (uint32_t)(lds_cu / lds);
				uint32_t by_waves = 2048u >> threads_shift;
				if (blocks > by_waves) blocks = by_waves;
				uint32_t waves = blocks << (threads_shift - 6);
				uint32_t balance = us > vs ? us - vs : vs - us;
				uint32_t score = (cc << 4) + (16 - balance);
				if (waves > best_waves || (waves == best_waves && score > best_score)) {
					best_waves = waves; best_score = score;
					q.u_shift = us; q.v_shift = vs; q.threads = 1u << threads_shift;
					q.channel_chunk = cc; q.lds_bytes = (uint32_t)lds;
				}
				if (cc == C) break;
			}
		}
	}
	if (!best_waves) return false;
	q.u_axis = (uint32_t)u_axis;
	q.depth_major = 1u;
	q.tiles[0] = blocks_at(a.size[u_axis], q.u_shift);
	q.tiles[1] = blocks_at(a.size[1 - u_axis], q.v_shift);
	q.tiles[2] = zcount;
	q.walk_columns = 1u;          /* the gather kernel: one column (four together doubled its HBM-side bytes at config 4, 280 -> 520 GB, time equal) */
	return true;
}

/* Upgrade a separable plan to the LDS-staged kernel (das_staged.hip) when the delay spread of a
 * tile provably fits the staging window.  The receive delay is a distance, so it changes by at
 * most one lateral voxel step (in samples) per voxel along u; the transmit delay likewise along
 * v, scaled by max|sin(angle)| when every transmit is a plane wave. */
static bool plan_staged(const BfDasArgs &a, const std::vector<BfTransmit> &tx, const float *xdc, const float *vox,
                        uint32_t zcount, BfSeparableArgs &q, bool allow_uniform = true)
{
	const Hooks &hk = hooks();
	const bool cplx = a.complex_data != 0;                       /* das_staged.hip / das_staged_real.hip */
	const bool cubic = a.interpolation == 2;                     /* das_staged_cubic.hip: complex samples only */
	if (a.interpolation != 1 && !(cubic && cplx)) return false;
	const uint32_t C = (uint32_t)a.channel_count, A = (uint32_t)a.acquisition_count;
	/* the kernels stage through 32-bit buffer offsets and park their padding loads at 2^31 */
	if ((uint64_t)C * A * (uint64_t)a.sample_count * (cplx ? 8u : 4u) >= (1ull << 31)) return false;
	const uint32_t A4 = (A + 3u) & ~3u;                          /* the kernel pads the transmit table to whole batches of 4 */
	const int u_axis = (int)q.u_axis, v_axis = 1 - u_axis;
	const int r = (tx[0].flags & BF_RX_ROWS) ? 1 : 0, w = (tx[0].flags & BF_TX_ROWS) ? 1 : 0;
	float m[16];
	m4_mul(xdc, vox, m);
	const float samples_per_metre = a.sampling_frequency * a.inv_speed_of_sound;
	float step_u = std::fabs(m[4 * u_axis + r]) / (float)(a.size[u_axis] > 1 ? a.size[u_axis] - 1 : 1) * samples_per_metre;
	float step_v = std::fabs(vox[4 * v_axis + w]) / (float)(a.size[v_axis] > 1 ? a.size[v_axis] - 1 : 1) * samples_per_metre;
	bool all_plane = true; float max_sin = 0.f;
	for (const BfTransmit &t : tx) {
		all_plane &= (t.flags & BF_TX_PLANE) != 0;
		max_sin = std::fmax(max_sin, std::fabs(t.sin_a));
	}
	if (tx[0].flags & BF_TX_NONE) step_v = 0.f;
	else if (all_plane)           step_v *= max_sin;

	const uint32_t lds_cu = 160u * 1024u;
	uint32_t best_waves = 0, best_score = 0;
	BfSeparableArgs best = q;
	for (uint32_t threads_shift = 10; threads_shift >= 9; threads_shift--) {
		for (uint32_t vs = 4; vs <= 6; vs++) {
			if (vs + 4 > threads_shift) continue;
			uint32_t us = threads_shift - vs;
			if (us > 6) continue;
			if ((u_axis == 0 ? us : vs) < 4) continue;
			float spread = step_u * (float)((1u << us) - 1) + step_v * (float)((1u << vs) - 1);
			if (!(spread >= 0.f && spread <= 60.f)) continue;                /* also a NaN / infinite spread (wild parameters) */
			uint32_t need = (uint32_t)std::ceil(spread * 1.001f) + (cubic ? 6 : 4);   /* + taps (k - 1 .. k + 2 for cubic), floors, rounding slack */
			uint32_t ws = need <= 32 ? 5 : need <= 64 ? 6 : 0;
			if (!ws) continue;
			/* hook STAGED_SHAPE="us,vs,ws": only this tile / window shape (testing every template instance;
			 * a window larger than needed is legal, a smaller one is not taken) */
			if (hk.staged_shape_set) {
				const unsigned fu = (unsigned)hk.staged_shape[0], fv = (unsigned)hk.staged_shape[1], fw = (unsigned)hk.staged_shape[2];
				if (fu != us || fv != vs) continue;
				if (fw < ws || fw > 6) continue;
				ws = fw;
			}
			/* complex samples, linear interpolation, x along the receive axis and a 64 x 16 tile: a wave's lanes share one row of the
			 * transmit axis, the transmit tables leave the LDS for a global table read through scalar loads (das_staged.hip, UNI).
			 * Measured faster than every other shape, so it is preferred wherever its window fits.  (An in-between
			 * 48-sample window for this form existed through round 3: 0.7 % faster at config 4 for 4 x the HBM-side traffic; removed.) */
			const bool uniform = allow_uniform && cplx && !cubic && u_axis == 0 && threads_shift == 10 && us == 6 && vs == 4 &&
			                     !hk.staged_nouniform;
			const uint32_t window = 1u << ws;
			/* window elements a thread stages per channel: 4 (complex: registers), 8 (real).  The linear kernels also rest their
			 * tap address on it -- one 16-bit shift of the element index: 4096 x 16 B and 8192 x 8 B both end at 64 KB */
			if (((uint64_t)A4 << ws) > ((uint64_t)(cplx ? 4 : 8) << threads_shift)) continue;
			const uint64_t stage_elements = (uint64_t)A4 * window;
			for (uint32_t chunk = 8; chunk <= 64; chunk *= 2) {
				uint32_t cc = chunk < C ? chunk : C;
				/* transmit tables 12 B per (transmit, v), receive table, {sample, difference} windows + a zero element, floors */
				uint64_t lds = cubic ? 12ull * ((uint64_t)A4 << vs) + 16ull * ((uint64_t)cc << us) + 32ull * (stage_elements + 3) + 4ull * (A4 + cc + 1) + 128
				             : cplx ? (uniform ? 0ull : 12ull * ((uint64_t)A4 << vs)) + 16ull * ((uint64_t)cc << us) + 16ull * (stage_elements + 3) + 4ull * (A4 + cc + 1) + 128
				                    :  4ull * ((uint64_t)A4 << vs) +  8ull * ((uint64_t)cc << us) +  8ull * (stage_elements + 4) + 4ull * (A4 + cc + 1) + 128;
				lds = (lds + 15) & ~15ull;
				if (lds > lds_cu) continue;
				uint32_t blocks = (uint32_t)(lds_cu / lds), by_waves = (cubic ? 1024u : 2048u) >> threads_shift;   /* (cubic: 128 VGPRs per lane) */
				if (blocks > by_waves) blocks = by_waves;
				uint32_t waves = blocks << (threads_shift - 6);
				uint32_t balance = us > vs ? us - vs : vs - us;
				uint32_t score = (blocks >= 2 ? 1000u : 0u) + (cc << 2) + (8 - balance) + (window == 32 ? 500u : 0u) +
				                 (uniform && window == 32 ? 2000u : 0u);
				if (waves > best_waves || (waves == best_waves && score > best_score)) {
					best_waves = waves; best_score = score;
					best.u_shift = us; best.v_shift = vs; best.threads = 1u << threads_shift;
					best.channel_chunk = cc; best.lds_bytes = (uint32_t)lds; best.window_shift = ws; best.window_samples = window;
					best.uniform = uniform ? 1u : 0u;
					best.table_stride = uniform ? 4u * A4 + 16u + 16u * (A4 / 4u) * 48u : 0u;
				}
				if (cc == C) break;
			}
		}
	}
	/* The plan is 32 x 32 tiles of 1024 threads with 32-sample windows (config 4: its spread does not fit a 64-wide tile's window):
	 * the channel-paired form of das_staged.hip, two voxels per lane (rows w, w + 16) and a wave's transmit rows shared, its transmit
	 * tables global as for the form above.  Same tiles, windows and chunk; the LDS holds two channels' windows of up to
	 * BF_STAGED_PAIRED_GROUP_MAX transmits at a time (in at most two groups here) instead of one channel's windows of all transmits
	 * and the transmit tables.  Decided by the shape alone: a slab takes the form the whole frame takes. */
	if (best_waves && allow_uniform && cplx && !cubic && !hk.staged_nouniform && best.threads == 1024 && best.u_shift == 5 && best.v_shift == 5 &&
	    best.window_samples == 32) {
		const uint32_t cc = best.channel_chunk;
		uint32_t g0, g1;
		/* the split (bf_kernels.h) fits the larger group beside the chunk's receive table in half a CU's LDS: two blocks per CU, as before */
		if (bf_staged_paired_split(A4, cc, &g0, &g1) && ((cc & 1u) == 0 || cc == C)) {
			const uint64_t lds = bf_staged_paired_lds_bytes(g0, cc, A4);
			best.uniform = 2u;
			best.lds_bytes = (uint32_t)lds;
			best.table_stride = 4u * A4 + 16u + 16u * (A4 / 2u) * 48u;
		}
	}
	if (hk.staged_checked) best.depth_major |= 2u;       /* test hook: the range-checked loop for every wave */
	/* global-table variants: the two blocks of a CU are neighbours along u in one plane (shared rows of the global transmit table) */
	if (best.uniform && (best.depth_major & 1u)) best.depth_major |= 4u;
	if (hk.debug)
		std::fprintf(stderr, "[beamformer] staged plan: step_u %.3f step_v %.3f waves %u u %u v %u w %u chunk %u lds %u uniform %u\n",
		             step_u, step_v, best_waves, best.u_shift, best.v_shift, best.window_samples, best.channel_chunk, best.lds_bytes, best.uniform);
	if (!best_waves) return false;
	q = best;
	q.tiles[0] = blocks_at(a.size[u_axis], q.u_shift);
	q.tiles[1] = blocks_at(a.size[v_axis], q.v_shift);
	q.tiles[2] = zcount;
	q.walk_columns = bf_walk_columns(q.tiles[0]);
	return true;
}

/* output rows (waves) per block of das_hercules.hip: they walk the outer elements in step.  Same-box A/B (gpurun_out/r04/ab_hbar2, round 4),
 * no barrier and 4 rows -> barrier and 4 / 8 / 16 rows: config 5 2896 -> 2705 / 2638 / 2888 ms, the reference harness's plane 18.46 -> 17.74 /
 * 17.47 / 19.43 ms, config 3 7.16 -> 7.18 / 7.26 / 7.55 ms */
static const uint32_t kHerculesRows = 8u;

/* Can this HERCULES-family frame use the aligned fast path (das_hercules.hip)?  The kernel lays
 * the 64 lanes of a wave along the output's x axis and reads the squared lateral distance along
 * the OTHER array axis from a per-output-row table, so one transducer lateral coordinate has to
 * be a function of the output row y alone: every product that would let voxel x or voxel z move
 * it must be an exact zero (then the table entry is bit-identical to the per-voxel value).
 * Everything else -- depth, the transmit distance, the coordinate along x -- stays per voxel. */
static bool plan_hercules(const BfDasArgs &a, const std::vector<BfTransmit> &tx, const float *xdc, const float *vox,
                          uint32_t zcount, bool forced, BfHerculesArgs &q)
{
	if (a.family != BF_DAS_HERCULES || tx.empty()) return false;
	if (!forced) {
		if (a.size[0] < 32 || a.split_shift) return false;       /* thin or tiny frames: the general kernel's channel split */
		if (((a.size[0] + 63u) & ~63u) > a.size[0] + a.size[0] / 3u) return false;   /* > 25 % idle lanes */
	}
	auto W = [&](int row, int col) { return vox[4 * col + row]; };
	auto X = [&](int row, int col) { return xdc[4 * col + row]; };
	/* does transducer coordinate `row` move with voxel axis `col`?  An axis of one voxel moves nothing, whatever its
	 * column of the transform holds: the view planes of math.c:844-885 keep their NORMAL there (das_transform_2d_xz: voxel z
	 * = (0, 1, 0), size 1), and the reference's own harness beamforms exactly such a plane (tests/throughput.c:20, :443-446) */
	auto moves = [&](int row, int col) {
		if (a.size[col] <= 1) return false;
		for (int k = 0; k < 3; k++) if (X(row, k) != 0.f && W(k, col) != 0.f) return true;
		return false;
	};
	int inner = -1;
	for (int coord = 0; coord < 2 && inner < 0; coord++)
		if (!moves(coord, 0) && !moves(coord, 2)) inner = coord;
	/* prefer the coordinate that does move with y when both qualify (a degenerate grid) */
	if (inner == 0 && !moves(1, 0) && !moves(1, 2) && !moves(0, 1) && moves(1, 1)) inner = 1;
	if (inner < 0) return false;
	const bool rx_cols = (tx[0].flags & BF_RX_COLUMNS) != 0;
	const int  tx_coord = rx_cols ? 1 : 0;                        /* das.glsl:238-247: transmit elements run along the other axis */
	const uint32_t A = (uint32_t)a.acquisition_count, C = (uint32_t)a.channel_count;
	const uint32_t transmits = A - (a.sparse ? 1u : 0u);
	if (!transmits || !C) return false;
	q.inner_coord       = (uint32_t)inner;
	q.inner_is_transmit = inner == tx_coord;
	q.inner_count       = q.inner_is_transmit ? transmits : C;
	q.outer_count       = q.inner_is_transmit ? C : transmits;
	q.table_pitch       = (q.inner_count + 8u + 3u) & ~3u;      /* the kernel prefetches one batch of 4 past the end */
	q.tiles[0] = (a.size[0] + 63u) / 64u;
	q.rows     = kHerculesRows;
	q.tiles[1] = (a.size[1] + q.rows - 1u) / q.rows;
	q.tiles[2] = zcount;
	{
		/* the axis along which the transducer-space depth changes fastest (as choose_tile finds it) */
		float m[16];
		m4_mul(xdc, vox, m);
		const uint32_t ext[3] = {a.size[0], a.size[1], zcount};
		int depth = 2; float best = -1.f;
		for (int i = 0; i < 3; i++) {
			if (ext[i] <= 1) continue;
			float step = std::fabs(m[4 * i + 2]) / (float)(a.size[i] > 1 ? a.size[i] - 1 : 1);
			if (step > best) { best = step; depth = i; }
		}
		q.depth_major = tile_walk(depth, zcount, q.tiles[1], q.band_rows);
	}
	/* unit of length: among the 8193 floats nearest 1, the s2 whose k' = float(k / sqrt(s2)) reproduces
	 * k = fs / c best as k' sqrt(s2) (errors are spread over +-3e-8, the best of 8193 lands near 1e-11).
	 * Remembered per (fs, c): frames of one plan ask again every launch. */
	{
		static float cached_fs = 0.f, cached_c = 0.f, cached_s2 = 1.f, cached_k = 0.f;
		if (cached_fs != a.sampling_frequency || cached_c != a.speed_of_sound) {
			const double k_exact = (double)a.sampling_frequency / (double)a.speed_of_sound;
			double best = 1e9;
			for (int i = -4096; i <= 4096; i++) {
				uint32_t bits = 0x3F800000u + (uint32_t)i;              /* floats around 1.0f in ulp steps */
				float s2; std::memcpy(&s2, &bits, sizeof s2);
				double s  = std::sqrt((double)s2);
				float  kk = (float)(k_exact / s);
				double err = std::fabs((double)kk * s / k_exact - 1.0);
				if (err < best) { best = err; cached_s2 = s2; cached_k = kk; }
			}
			cached_fs = a.sampling_frequency; cached_c = a.speed_of_sound;
		}
		q.unit_scale2 = cached_s2; q.samples_per_unit = cached_k;
	}
	{
		/* distances to two elements of the inner axis differ by at most their separation: at most 255 pitches (dense or
		 * sparse element indices alike), i.e. this many turns of demodulation phase inside one inner loop */
		const float span_turns = std::fabs(a.turns_per_sample) * 255.0f * std::fabs(a.pitch[inner]) * a.sampling_frequency * a.inv_speed_of_sound;
		q.phase_local = a.complex_data && span_turns < 400.0f;         /* (false for a NaN) */
	}
	return true;
}

/* Can the per-voxel factored kernel (das_factored.hip) take this frame?  It needs the sample
 * index to be a receive term plus a transmit term: RCA-family frames whose transmits all share
 * one receive orientation, and FORCES/UFORCES.  With fewer than three transmits per channel
 * chunk the receive factors are not amortised and the general kernel is as fast. */
static bool factored_applies(const BfDasArgs &a, const std::vector<BfTransmit> &tx, uint32_t request)
{
	if (request == BeamformerHipDasPath_General) return false;
	int transmits = a.acquisition_count - (a.family == BF_DAS_FORCES && a.sparse ? 1 : 0);
	if (transmits < 3 && request != BeamformerHipDasPath_PreferFactored) return false;
	if (a.family == BF_DAS_FORCES) return true;
	if (a.family != BF_DAS_RCA || tx.empty()) return false;
	for (const BfTransmit &t : tx)
		if ((t.flags & BF_RX_ROWS) != (tx[0].flags & BF_RX_ROWS)) return false;
	return true;
}

/* ---------------------------------------------------------------- the decision */

std::vector<BfTransmit> build_transmit_table(const ParameterBlock &pb)
{
	const BeamformerParameters &bp = pb.parameters;
	const uint32_t A = bp.acquisition_count;
	std::vector<BfTransmit> table(A, BfTransmit{});
	for (uint32_t a = 0; a < A; a++) {
		uint32_t txrx  = bp.single_orientation ? (bp.transmit_receive_orientation & 0xFFu) : pb.transmit_receive_orientations[a];
		float    angle = bp.single_focus ? bp.focal_vector[0] : pb.focal_vectors[a][0];
		float    depth = bp.single_focus ? bp.focal_vector[1] : pb.focal_vectors[a][1];
		uint32_t tx = (txrx >> 4) & 0xF, rx = txrx & 0xF;
		BfTransmit &t = table[a];
		float rad = angle * 0.017453292519943295f;               /* GLSL radians() */
		t.sin_a = sinf(rad); t.cos_a = cosf(rad);
		t.flags = 0;
		if (tx == BeamformerRCAOrientation_None)    t.flags |= BF_TX_NONE;
		if (tx == BeamformerRCAOrientation_Rows)    t.flags |= BF_TX_ROWS;
		if (rx == BeamformerRCAOrientation_Rows)    t.flags |= BF_RX_ROWS;
		if (rx == BeamformerRCAOrientation_Columns) t.flags |= BF_RX_COLUMNS;
		if (std::isinf(depth)) { t.flags |= BF_TX_PLANE; t.focus_x = t.focus_z = 0; }
		else                   { t.focus_x = depth * t.sin_a; t.focus_z = depth * t.cos_a; }
	}
	return table;
}

/* voxel (unit cube) -> transducer coordinates of a family's frames: FORCES and READI plans carry the product already (plan_on_view) */
static void voxel_to_xdc(int family, const ParameterBlock &pb, const Plan &plan, float *m)
{
	if (family == BF_DAS_FORCES || family == BF_DAS_READI) std::memcpy(m, plan.das_voxel_transform, sizeof(plan.das_voxel_transform));
	else m4_mul(pb.parameters.xdc_transform, plan.das_voxel_transform, m);
}

/* What the rules of decide_das share: the frame they judge, the decision they fill, and what fill_das_args found on its way */
struct Frame {
	const ParameterBlock &pb; const Plan &plan; const std::vector<BfTransmit> &tx;
	uint32_t mode, request;              /* the das path mode word; its kernel request (das_path_request) */
	DasDecision &out;                    /* out.z_first, out.z_count: the planes of this launch */
	float    to_xdc[16];                 /* voxel_to_xdc of the frame's family */
	uint32_t ext[3];                     /* voxels of this launch per axis */
	bool     factored;                   /* factored_applies */
};

/* out.a, out.general, out.das_input_bytes and out.depth_axis from block, plan and mode: every argument of the general kernel, its tile
 * and channel split included.  It chooses no kernel: the rules behind it do, and change what their kernels read otherwise. */
static void fill_das_args(Frame &f)
{
	const ParameterBlock &pb = f.pb; const Plan &plan = f.plan; DasDecision &out = f.out;
	const BeamformerParameters &bp = pb.parameters;
	const uint32_t zfirst = out.z_first, zcount = out.z_count, mode = f.mode;
	const uint32_t C = plan.channels, A = plan.acquisitions, Sd = plan.das_samples;

	BfDasArgs &a = out.a;
	std::memcpy(a.xdc_transform,   bp.xdc_transform,         sizeof(a.xdc_transform));
	std::memcpy(a.voxel_transform, plan.das_voxel_transform, sizeof(a.voxel_transform));
	a.pitch[0] = bp.xdc_element_pitch[0]; a.pitch[1] = bp.xdc_element_pitch[1];
	switch (bp.acquisition_kind) {                                          /* das.glsl:381-400 */
	case BeamformerAcquisitionKind_FORCES:
	case BeamformerAcquisitionKind_UFORCES:
		a.family = bp.readi_group_count > 1 ? BF_DAS_READI : BF_DAS_FORCES; break;
	case BeamformerAcquisitionKind_HERCULES:
	case BeamformerAcquisitionKind_UHERCULES:
	case BeamformerAcquisitionKind_HERO_PA:
		a.family = BF_DAS_HERCULES; break;
	case BeamformerAcquisitionKind_Flash:
	case BeamformerAcquisitionKind_RCA_TPW:
	case BeamformerAcquisitionKind_RCA_VLS:
		a.family = BF_DAS_RCA; break;
	default: a.family = -1; break;      /* the shader leaves the voxel at zero */
	}
	a.interpolation = (int32_t)bp.interpolation_mode;
	a.complex_data  = plan.iq_pipeline;
	a.coherency_weighting = bp.coherency_weighting != 0;
	a.acquisition_count = (int32_t)A; a.channel_count = (int32_t)C; a.sample_count = (int32_t)Sd;
	a.sparse = plan.das_sparse;
	a.sampling_frequency     = plan.das_sampling_frequency;
	a.inv_sampling_frequency = 1.0f / plan.das_sampling_frequency;
	a.demodulation_frequency = bp.demodulation_frequency;
	a.inv_speed_of_sound     = 1.0f / bp.speed_of_sound;
	a.speed_of_sound         = bp.speed_of_sound;
	a.turns_per_sample       = bp.demodulation_frequency * a.inv_sampling_frequency;
	a.first_transmit_weight  = 1.0f / sqrtf((float)A);
	a.time_offset = plan.das_time_offset;
	a.f_number    = bp.f_number;
	/* das_exact.h: how close to an end of an RF row a kernel may still trust its own index.  The index is a sum of terms of magnitude
	 * up to M = S + |t0 fs| (distance terms and the time offset), each rounded a few times on its way: the kernels' indices and the
	 * shader's differ by a few ulp(M) = M 2^-23 (measured bound: the out-of-sample fuzz, profiles/r04_fuzz.json, runs with this margin).  The
	 * margin is M 2^-19 -- 16 ulp(M): 2^-10 sample for 512-sample rows, 2^-8 for 2048 --, never under 2^-11. */
	{
		const float magnitude = (float)Sd + std::fabs(plan.das_time_offset * plan.das_sampling_frequency);
		a.edge_margin = std::fmax(std::ldexp(magnitude, -19), std::ldexp(1.0f, -11));
		if (!(a.edge_margin < 0.25f)) a.edge_margin = 0.25f;        /* (wild parameters; also a NaN) */
	}
	a.size[0] = plan.output_points[0]; a.size[1] = plan.output_points[1]; a.size[2] = plan.output_points[2];
	a.z_first = zfirst; a.z_count = zcount;
	a.readi_group_count = bp.readi_group_count; a.readi_group = bp.readi_group;
	out.das_input_bytes = (uint64_t)C * A * Sd * (plan.iq_pipeline ? 8u : 4u);

	float (&to_xdc)[16] = f.to_xdc;
	uint32_t (&ext)[3] = f.ext;
	voxel_to_xdc(a.family, pb, plan, to_xdc);
	ext[0] = a.size[0]; ext[1] = a.size[1]; ext[2] = zcount;
	/* Small frames (real-time 2-D imaging) do not fill 256 CUs with one thread per voxel:
	 * split the channel loop over K waves of a block (wave-level partial sums, combined
	 * through LDS in split order) until the launch has ~16 waves per CU (config 1, us per
	 * frame by target wave count: 2048 -> 19.9, 4096 -> 15.2, 8192 -> 15.1, 16384 -> 17.1). */
	const uint64_t voxel_waves = ((uint64_t)ext[0] * ext[1] * ext[2] + 63) / 64;
	a.split_shift = 0;
	const uint64_t split_target = 4096;
	while (!(mode & BeamformerHipDasPath_NoChannelSplit) && a.split_shift < 4 && (voxel_waves << a.split_shift) < split_target && (C >> (a.split_shift + 1)) >= 4) a.split_shift++;
	out.depth_axis = choose_tile(to_xdc, a.size, zcount, a.tile_shift, a.split_shift ? 6 : 8);
	for (int k = 0; k < 3; k++) a.blocks[k] = blocks_at(ext[k], a.tile_shift[k]);
	a.depth_major = tile_walk(out.depth_axis, zcount, a.blocks[1], a.band_rows);
	out.general = a;
}

/* ---- the rules.  Each returns whether it took the frame.  The reason a path declines with has ONE writer: its rule, or the *_declines
 * function its rule shares with a rule in front that took the frame and speaks for it. */

static const char *const kGeneralAsked = "das path 1: the general kernel was asked for";

static bool take(Frame &f, int path)      /* a specialised kernel runs the frame */
{
	f.out.path = path;
	f.out.why[DasPath_General] = "a specialised kernel applies";
	return true;
}

static bool rule_zero(Frame &f)
{
	const BfDasArgs &a = f.out.a;
	if (a.family >= 0 && a.interpolation >= 0 && a.interpolation <= 2) return false;
	for (auto &w : f.out.why) w = "acquisition kind or interpolation mode the shader leaves at zero";
	f.out.path = DasPath_Zero;
	return true;
}

static void hercules_declines(Frame &f)
{
	f.out.why[DasPath_Hercules] = f.request == BeamformerHipDasPath_General ? kGeneralAsked
	                            : f.out.a.family != BF_DAS_HERCULES ? "not a HERCULES-family acquisition"
	                            : f.out.a.split_shift ? "a small frame: the general kernel's channel split fills the chip better"
	                            : "grid narrower than 32 voxels along x / more than 25 % idle lanes, or no transducer axis is a function of the output row alone";
}

static void factored_declines(Frame &f)
{
	const int family = f.out.a.family;
	f.out.why[DasPath_Factored] = f.request == BeamformerHipDasPath_General ? kGeneralAsked
	                            : family == BF_DAS_HERCULES || family == BF_DAS_READI ? "the sample index is not a receive term plus a transmit term (HERCULES / READI)"
	                            : "fewer than 3 transmits per channel chunk, or transmits with different receive orientations";
}

/* das_separable.hip (gather) and das_staged*.hip (staged): why[Gather] and why[Staged] */
static bool rule_separable(Frame &f)
{
	DasDecision &out = f.out;
	const BfDasArgs &a = out.a;
	const Plan &plan = f.plan;
	const float *xdc = f.pb.parameters.xdc_transform, *vox = plan.das_voxel_transform;
	auto &why = out.why;
	if (f.request == BeamformerHipDasPath_General || f.request == BeamformerHipDasPath_PreferFactored) {
		why[DasPath_Gather] = why[DasPath_Staged] = f.request == BeamformerHipDasPath_General ? kGeneralAsked : "das path 4: the factored kernel was asked for";
		return false;
	}
	BfSeparableArgs sep{};
	if (!plan_separable(a, f.tx, xdc, vox, out.z_count, sep)) {
		why[DasPath_Gather] = why[DasPath_Staged] = "not a row-column frame whose receive and transmit delays separate over the voxel x / y axes with depth on z";
		return false;
	}
	/* The LDS-table kernels' hand-scheduled loop exists for linear interpolation; for cubic and nearest the gather kernel's
	 * generic loop loses to the factored kernel (200 ch x 33 tx -> 129 x 333 x 21, cubic: 7.6 ms against 4.8 ms; nearest 2.6
	 * against 2.1), which then goes first -- except for cubic IQ frames with enough transmits, which try the staged cubic kernel
	 * (it declines, and the factored kernel runs, when the geometry is not separable or the spread does not fit a window). */
	const bool prefer_staged = f.request == BeamformerHipDasPath_PreferLdsStaged;
	const bool want_staged   = prefer_staged || (f.request == BeamformerHipDasPath_Automatic && plan.acquisitions >= kStagedMinTransmits);
	const bool staged_cubic  = a.interpolation == 2 && plan.iq_pipeline && want_staged;
	bool tables_first = a.interpolation == 1 || prefer_staged || staged_cubic || !f.factored;
	sep.zero_offset = (uint32_t)out.das_input_bytes;                                /* 64 zero bytes right behind the DAS input */
	const BfSeparableArgs gather = sep;
	bool staged = false;
	if (!want_staged) {
		why[DasPath_Staged] = f.request == BeamformerHipDasPath_NoLdsStaging ? "das path 2: no LDS staging"
		                    : "fewer than 6 transmits per channel: two barriers and a window copy per channel are not amortised";
	} else {
		staged = plan_staged(a, f.tx, xdc, vox, out.z_count, sep);
		if (!staged) {
			sep = gather;
			why[DasPath_Staged] = a.interpolation == 0 ? "nearest interpolation" : (a.interpolation == 2 && !plan.iq_pipeline) ? "cubic interpolation of real samples"
			                    : out.das_input_bytes >= (1ull << 31) ? "DAS input of 2 GiB or more (32-bit staging offsets)"
			                    : "the delay spread of no tile shape fits a 32- / 64-sample window (or the windows do not fit the LDS)";
		}
	}
	if (!staged && staged_cubic && !prefer_staged && f.factored) tables_first = false;      /* cubic: the factored kernel, not the gather kernel's generic loop */
	if (!staged && !tables_first) {
		why[DasPath_Gather] = "cubic / nearest interpolation: its generic loop loses to the factored kernel";
		return false;
	}
	out.sep = sep; out.sep_gather = gather;
	take(f, staged ? DasPath_Staged : DasPath_Gather);
	if (staged && sep.uniform) {
		/* the wave-uniform transmit tables live in global memory (a few MB to 244 MB at 512^3 with 75 transmits); too big or no
		 * memory at launch: the shape with the tables in LDS, planned here */
		BfSeparableArgs again = gather;
		out.has_lds_tables = plan_staged(a, f.tx, xdc, vox, out.z_count, again, false);
		if (out.has_lds_tables) out.sep_lds_tables = again;
		const uint64_t table_bytes = (uint64_t)sep.table_stride * sep.tiles[1] * sep.tiles[2];
		if (table_bytes > hooks().staged_table_cap) {
			if (out.has_lds_tables) out.sep = again;
			else { out.sep = gather; out.path = DasPath_Gather; why[DasPath_Staged] = "global transmit table too large and no LDS-table shape fits"; }
		}
	}
	if (out.path == DasPath_Staged) why[DasPath_Gather] = "superseded by the LDS-staged kernel";
	/* the rules behind it: a row-column frame is no HERCULES frame; the factored kernel would have run it, or says why not */
	hercules_declines(f);
	if (f.factored) why[DasPath_Factored] = "superseded by the separable-delay kernels";
	return true;
}

/* das_hercules.hip: why[Hercules] */
static bool rule_hercules(Frame &f)
{
	DasDecision &out = f.out;
	const BfDasArgs &a = out.a;
	BfHerculesArgs hq{};
	if (f.request == BeamformerHipDasPath_General ||
	    !plan_hercules(a, f.tx, f.pb.parameters.xdc_transform, f.plan.das_voxel_transform, out.z_count, f.request == BeamformerHipDasPath_HerculesAnyWidth, hq)) {
		hercules_declines(f);
		return false;
	}
	hq.zero_offset = (uint32_t)out.das_input_bytes;
	/* linear / cubic interpolation of IQ samples may read a prepared copy of the input ({sample, difference}, 16 bytes; cubic: the
	 * four polynomial coefficients of every segment, 32 bytes; 32-bit byte offsets: under 4 GiB).  Not on coarse grids: the copy
	 * is 2-4 x the RF, and where every lane reads its own cache line the memory system pays for the bytes -- the harness's view
	 * plane with cubic polynomials: 28.1 ms, 158 GB from beyond L2 per frame; with the taps gathered from the RF itself 25.2 ms */
	const uint64_t prepared = out.das_input_bytes * (a.interpolation == 2 ? 4u : 2u);
	out.hercules_prepared = f.plan.iq_pipeline && (a.interpolation == 1 || a.interpolation == 2) && prepared + 64 < (1ull << 32) &&
	                        lane_step_samples(f.to_xdc, a) < 1.0f;
	out.herc = hq;
	/* (the factored rule behind it has said why not: f.factored is false for this family) */
	return take(f, DasPath_Hercules);
}

/* das_tile.hip: why[Tile].  Cubic IQ frames on FINE grids -- there the four taps of a term are two gather instructions through L1 (32.6 clk
 * per CU per term: what config 2 waits for) and a 64 x 16-voxel block touches a window of a few dozen samples of every RF row, which
 * the block stages as cubic polynomials.  Tried when the estimated spread of such a tile fits a 64-sample window (the kernel measures
 * the real spread per block and chunk and falls back to the gather loop itself, so the estimate only decides whether it is worth
 * trying); flag 0x100 forces it wherever it is supported, 0x200 forbids it. */
static bool rule_tile(Frame &f)
{
	if (!f.factored) return false;          /* (why[Tile] keeps what decide_das gave it) */
	DasDecision &out = f.out;
	BfDasArgs &a = out.a;
	const Plan &plan = f.plan;
	const uint32_t (&ext)[3] = f.ext;
	bool tile_ok = plan.iq_pipeline && a.interpolation == 2 && plan.das_samples >= 8 && out.das_input_bytes < (1ull << 31) &&
	               plan.acquisitions - (a.family == BF_DAS_FORCES && a.sparse ? 1u : 0u) >= 4u;
	/* tile: 64 voxels along x (a wave), the other 16 along the next axis that has voxels */
	uint32_t shift[3] = {0, 0, 0}, left = 10;
	for (int k = 0; k < 3 && left; k++) {
		uint32_t room = ceil_log2(ext[k]), want = k == 0 ? 6u : left;
		uint32_t give = room < want ? room : want;
		give = give < left ? give : left;
		shift[k] = give; left -= give;
	}
	for (int k = 0; k < 3 && left; k++) { uint32_t room = ceil_log2(ext[k]) - shift[k]; uint32_t give = room < left ? room : left; shift[k] += give; left -= give; }
	/* (left > 0: a frame -- or a device's slab of it -- that does not even span one 1024-voxel tile) */
	/* the derivative bound first (cheap, a true upper bound); where it does not already say "32 samples", what the kernel would measure
	 * on the image's extreme tiles */
	float spread = tile_spread_estimate(a, f.tx, f.to_xdc, plan.das_voxel_transform, shift);
	if (left == 0 && spread == spread && spread > 26.f && spread < 400.f) {
		const float sampled = tile_spread_sampled(a, f.tx, f.pb, plan.das_voxel_transform, ext, shift, out.z_first);
		if (sampled == sampled && sampled < spread) spread = sampled;
	}
	out.tile_spread = left == 0 ? spread : 0.f;
	for (int k = 0; k < 3; k++) out.tile_estimate_shift[k] = shift[k];
	/* frames small enough for the channel split (under 4096 voxel waves): one block per CU, so the block-staged kernel is
	 * only worth it from about three quarters of the CUs (config 2 onto 448 x 448: 196 blocks, 0.66 ms against the split
	 * kernel's 0.82; onto 384 x 384 the split kernel wins: profiles/r03_tile_threshold.json) */
	uint64_t tile_blocks = 1;
	for (int k = 0; k < 3; k++) tile_blocks *= blocks_at(ext[k], shift[k]);
	tile_ok = tile_ok && (!a.split_shift || tile_blocks >= 192u);
	const bool forced = (f.mode & BeamformerHipDasPath_TileStaging) != 0, forbidden = (f.mode & BeamformerHipDasPath_NoTileStaging) != 0;
	if (!(tile_ok && left == 0 && !forbidden && (forced || (spread == spread && spread <= 58.f && lane_step_samples(f.to_xdc, a) < 1.0f)))) {
		out.why[DasPath_Tile] = !plan.iq_pipeline || a.interpolation != 2 ? "cubic interpolation of IQ samples only"
		                      : !tile_ok ? "small frame (channel split: fewer than 192 blocks), fewer than 4 transmits, or a DAS input of 2 GiB or more"
		                      : forbidden ? "das path flag 0x200: no block staging"
		                      : "coarse grid or steep delays: a 64 x 16-voxel tile's estimated spread exceeds a 64-sample window";
		return false;
	}
	a.zero_offset = (uint32_t)out.das_input_bytes;
	a.split_shift = 0;
	for (int k = 0; k < 3; k++) a.tile_shift[k] = shift[k];
	for (int k = 0; k < 3; k++) a.blocks[k] = blocks_at(ext[k], a.tile_shift[k]);
	a.depth_major = tile_walk(out.depth_axis, out.z_count, a.blocks[1], a.band_rows);
	a.tile_window_shift = spread <= 26.f ? 5u : 6u;
	out.why[DasPath_Factored] = "superseded by its block-staged form (das_tile.hip)";      /* the rule behind it */
	return take(f, DasPath_Tile);
}

/* das_factored.hip: why[Factored] (factored_declines: decide_das, before the ladder -- the separable rule orders itself by f.factored) */
static bool rule_factored(Frame &f)
{
	if (!f.factored) return false;
	f.out.a.zero_offset = (uint32_t)f.out.das_input_bytes;
	return take(f, DasPath_Factored);
}

/* das.hip: the fallback declines nothing (why[General]: take) */
static bool rule_general(Frame &f) { f.out.path = DasPath_General; return true; }

void decide_das(const ParameterBlock &pb, const Plan &plan, const std::vector<BfTransmit> &tx,
                uint32_t zfirst, uint32_t zcount, uint32_t mode, DasDecision &out)
{
	out = DasDecision{};
	out.z_first = zfirst; out.z_count = zcount; out.mode = mode; out.hooks_version = hooks().version;
	Frame f{pb, plan, tx, mode, das_path_request(mode), out, {}, {}, false};
	fill_das_args(f);
	out.valid = true;
	if (rule_zero(f)) return;
	out.why[DasPath_Tile] = "only where the factored kernel would run (its block-staged form)";      /* (a frame das_tile.hip takes keeps it) */
	f.factored = factored_applies(out.a, tx, f.request);
	if (!f.factored) factored_declines(f);
	if (rule_separable(f)) return;
	if (rule_hercules(f)) return;
	if (rule_tile(f)) return;
	if (rule_factored(f)) return;
	rule_general(f);
}


/* ---------------------------------------------------------------- row ends (das_exact.h), host side */

namespace {

struct Range { double lo, hi; };

/* smallest and largest |v| of values v in [lo, hi] */
Range abs_range(double lo, double hi)
{
	if (lo <= 0 && hi >= 0) return {0.0, std::fmax(-lo, hi)};
	return {std::fmin(std::fabs(lo), std::fabs(hi)), std::fmax(std::fabs(lo), std::fabs(hi))};
}

double point_segment_distance(double px, double py, double ax, double ay, double bx, double by)
{
	const double vx = bx - ax, vy = by - ay, wx = px - ax, wy = py - ay;
	const double vv = vx * vx + vy * vy;
	double t = vv > 0 ? (wx * vx + wy * vy) / vv : 0.0;
	t = t < 0 ? 0 : (t > 1 ? 1 : t);
	const double dx = ax + t * vx - px, dy = ay + t * vy - py;
	return std::sqrt(dx * dx + dy * dy);
}

/* Bounds on the sample index of every IN-APERTURE term of plane z (whole grid coordinates), for the families the staged kernels take
 * (RCA with one receive orientation; FORCES).  Voxel -> world -> transducer is affine, so coordinates take their extremes at the
 * plane's corners; distances to points are convex (largest at a corner) and bounded below by the distance to the corners' hull. */
Range plane_index_bounds(const BfDasArgs &a, const std::vector<BfTransmit> &tx, const float *vox, const float *to_xdc,
                         const int16_t *sparse_elements, uint32_t z)
{
	double world[4][3], xdc[4][3];
	const double pz = (double)z / (double)(a.size[2] > 1 ? a.size[2] - 1 : 1);
	for (int k = 0; k < 4; k++) {
		const double px = (k & 1) && a.size[0] > 1 ? 1.0 : 0.0, py = (k & 2) && a.size[1] > 1 ? 1.0 : 0.0;
		for (int i = 0; i < 3; i++) {
			world[k][i] = vox[i] * px + vox[4 + i] * py + vox[8 + i] * pz + vox[12 + i];
			xdc[k][i]   = to_xdc[i] * px + to_xdc[4 + i] * py + to_xdc[8 + i] * pz + to_xdc[12 + i];
		}
	}
	auto over_corners = [&](auto f) { Range r{1e300, -1e300}; for (int k = 0; k < 4; k++) { double v = f(k); r.lo = std::fmin(r.lo, v); r.hi = std::fmax(r.hi, v); } return r; };
	const bool forces = a.family == BF_DAS_FORCES;
	const int  r_axis = forces ? 0 : ((tx[0].flags & BF_RX_ROWS) ? 1 : 0);
	const Range zr = over_corners([&](int k) { return xdc[k][2]; });
	const Range za = abs_range(zr.lo, zr.hi);
	/* receive: |dx| < |z| / (2 F#) inside the aperture, and never beyond what the array and the plane allow */
	auto reach_along = [&](int axis) {
		const Range lat = over_corners([&](int k) { return xdc[k][axis]; });
		const double last = (double)(a.channel_count - 1) * (double)a.pitch[axis];
		return std::fmax(std::fmax(std::fabs(lat.lo), std::fabs(lat.hi)), std::fmax(std::fabs(lat.lo - last), std::fabs(lat.hi - last)));
	};
	double dx_max = reach_along(r_axis);
	if (!forces && a.family == BF_DAS_RCA)
		for (const BfTransmit &t : tx)                          /* per-transmit receive orientations (general kernel): the larger reach */
			if (((t.flags & BF_RX_ROWS) ? 1 : 0) != r_axis) { dx_max = std::fmax(dx_max, reach_along(1 - r_axis)); break; }
	if (a.f_number > 0) dx_max = std::fmin(dx_max, 0.5 * za.hi / (double)a.f_number);
	const double rx_max = std::sqrt(dx_max * dx_max + za.hi * za.hi), rx_min = za.lo;
	const double c = a.speed_of_sound, fs = a.sampling_frequency, t0 = a.time_offset;
	Range index{1e300, -1e300};
	/* das.glsl:187-202 over the plane: a plane wave's "distance" is affine (extremes at the corners); a focused or diverging wave's is
	 * the distance to the focus: largest at a corner, smallest zero if the focus lies inside the (px, pz) image of the plane, else the
	 * distance to its boundary (corner order 0, 1, 3, 2 walks the parallelogram) */
	auto transmit_range = [&](const BfTransmit &t) {
		Range d{0.0, 0.0};
		if (t.flags & BF_TX_NONE) return d;
		const int w = (t.flags & BF_TX_ROWS) ? 1 : 0;
		if (t.flags & BF_TX_PLANE) return over_corners([&](int k) { return world[k][w] * (double)t.sin_a + world[k][2] * (double)t.cos_a; });
		d = over_corners([&](int k) { return std::hypot(world[k][w] - (double)t.focus_x, world[k][2] - (double)t.focus_z); });
		const int order[4] = {0, 1, 3, 2};
		double nearest = 1e300; int sign = 0; bool inside = true;
		for (int e = 0; e < 4; e++) {
			const int i = order[e], j = order[(e + 1) & 3];
			nearest = std::fmin(nearest, point_segment_distance(t.focus_x, t.focus_z, world[i][w], world[i][2], world[j][w], world[j][2]));
			const double cross = (world[j][w] - world[i][w]) * ((double)t.focus_z - world[i][2]) - (world[j][2] - world[i][2]) * ((double)t.focus_x - world[i][w]);
			if (cross != 0) { const int sg = cross > 0 ? 1 : -1; if (sign && sg != sign) inside = false; sign = sg; }
		}
		d.lo = (inside && sign) ? 0.0 : nearest;
		return d;
	};
	if (a.family == BF_DAS_HERCULES) {
		/* das.glsl:233-286: index = T0(voxel) + sqrt(z^2 + e^2) fs / c over element pairs with e^2 < z^2 / (4 F#^2); without an f-number
		 * every pair passes: e^2 then is bounded by the array (both lateral axes) */
		double e_max;
		if (a.f_number > 0) e_max = 0.5 * za.hi / (double)a.f_number;
		else {
			const Range lx = over_corners([&](int k) { return xdc[k][0]; }), ly = over_corners([&](int k) { return xdc[k][1]; });
			const double n = (double)(a.channel_count > a.acquisition_count ? a.channel_count : a.acquisition_count) + 1.0;
			double far_x = std::fabs(n * a.pitch[0]), far_y = std::fabs(n * a.pitch[1]);
			if (a.sparse) for (int t = 0; t + 1 < a.acquisition_count; t++) { far_x = std::fmax(far_x, std::fabs((double)sparse_elements[t] * a.pitch[0])); far_y = std::fmax(far_y, std::fabs((double)sparse_elements[t] * a.pitch[1])); }
			const double ex = std::fmax(std::fabs(lx.lo), std::fabs(lx.hi)) + far_x, ey = std::fmax(std::fabs(ly.lo), std::fabs(ly.hi)) + far_y;
			e_max = std::sqrt(ex * ex + ey * ey);
		}
		const Range d = transmit_range(tx[0]);
		index.lo = (d.lo / c + t0) * fs + za.lo * fs / c;
		index.hi = (d.hi / c + t0) * fs + std::sqrt(za.hi * za.hi + e_max * e_max) * fs / c;
		return index;
	}
	if (forces) {
		/* das.glsl:288-321: every decoded transmit element e: sqrt((y - pitch_y C / 2)^2 + z^2 + (x - pitch_x e)^2) */
		const double half = (double)a.pitch[1] * (double)a.channel_count / 2.0;
		const Range ty = over_corners([&](int k) { return xdc[k][1] - half; });
		const Range tya = abs_range(ty.lo, ty.hi);
		double e_lo = a.sparse ? 1e300 : 0.0, e_hi = a.sparse ? -1e300 : (double)(a.acquisition_count - 1);
		if (a.sparse) for (int t = 0; t + 1 < a.acquisition_count; t++) { e_lo = std::fmin(e_lo, sparse_elements[t]); e_hi = std::fmax(e_hi, sparse_elements[t]); }
		const Range xs = over_corners([&](int k) { return xdc[k][0]; });
		const Range txa = abs_range(xs.lo - (double)a.pitch[0] * (a.pitch[0] >= 0 ? e_hi : e_lo), xs.hi - (double)a.pitch[0] * (a.pitch[0] >= 0 ? e_lo : e_hi));
		const double tx_max = std::sqrt(tya.hi * tya.hi + za.hi * za.hi + txa.hi * txa.hi);
		const double tx_min = std::sqrt(tya.lo * tya.lo + za.lo * za.lo + txa.lo * txa.lo);
		index.lo = (rx_min / c + t0) * fs + tx_min * fs / c;
		index.hi = (rx_max / c + t0) * fs + tx_max * fs / c;
		return index;
	}
	for (const BfTransmit &t : tx) {
		const Range d = transmit_range(t);
		index.lo = std::fmin(index.lo, ((d.lo + rx_min) / c + t0) * fs);
		index.hi = std::fmax(index.hi, ((d.hi + rx_max) / c + t0) * fs);
	}
	return index;
}

} // namespace

/* the mode the planes of a row-end fallback part are decided under: the caller's flags, block staging off, kernel request `request` */
static uint32_t row_end_fallback_mode(uint32_t mode, uint32_t request)
{
	return (mode & ~kDasPathRequestMask & ~(uint32_t)BeamformerHipDasPath_TileStaging) | BeamformerHipDasPath_NoTileStaging | request;
}

void decide_das_parts(const ParameterBlock &pb, const Plan &plan, const std::vector<BfTransmit> &tx,
                      uint32_t zfirst, uint32_t zcount, uint32_t mode, std::vector<DasDecision> &parts)
{
	parts.clear();
	parts.emplace_back();
	decide_das(pb, plan, tx, zfirst, zcount, mode, parts[0]);
	DasDecision &whole = parts[0];
	whole.a.row_ends = whole.general.row_ends = 1;           /* until shown otherwise */
	if (whole.path == DasPath_Zero || zcount == 0 || tx.empty()) return;
	const BfDasArgs &a = whole.a;
	/* a bound exists for the families whose index is a sum of distances over an aperture the f-number limits (plane_index_bounds);
	 * READI keeps row_ends = 1, and so does nearest interpolation (which has no row-end evaluation: its flips are everywhere) */
	if (a.family == BF_DAS_READI || a.family < 0 || a.interpolation == 0) return;
	float to_xdc[16];
	voxel_to_xdc(a.family, pb, plan, to_xdc);
	const bool   cubic = a.interpolation == 2;
	const double reach = 2.0 * (double)a.edge_margin;        /* the kernels' indices and these bounds differ by far less than the margin */
	const double lo = (cubic ? 1.0 : 0.0) + reach, hi = (double)(a.sample_count - (cubic ? 2 : 1)) - reach;
	std::vector<uint8_t> clear(zcount);
	bool all = true;
	for (uint32_t k = 0; k < zcount; k++) {
		const Range r = plane_index_bounds(a, tx, plan.das_voxel_transform, to_xdc, pb.sparse_elements, zfirst + k);
		clear[k] = r.lo >= lo && r.hi < hi;                  /* (false for a NaN) */
		if (hooks().debug && (k == 0 || k + 1 == zcount))
			std::fprintf(stderr, "[beamformer] row ends: plane %u index within [%.3f, %.3f], clear within [%.3f, %.3f): %s\n", zfirst + k, r.lo, r.hi, lo, hi, clear[k] ? "clear" : "fallback");
		all = all && clear[k];
	}
	if (all) { whole.a.row_ends = whole.general.row_ends = 0; return; }      /* no term of this launch comes near a row end */
	if (whole.path != DasPath_Staged && whole.path != DasPath_Tile) return;    /* every other kernel evaluates such terms itself */
	/* the kernel behind the staged one, with block staging off: the one asked for where it evaluates row ends itself (1: general,
	 * 4: factored), else "automatic, never staged" (a request for the LDS-staged kernel, 3, included) */
	const uint32_t asked = das_path_request(mode);
	const bool exact_asked = asked == BeamformerHipDasPath_General || asked == BeamformerHipDasPath_PreferFactored;
	const uint32_t fallback_mode = row_end_fallback_mode(mode, exact_asked ? asked : (uint32_t)BeamformerHipDasPath_NoLdsStaging);
	std::vector<DasDecision> cut;
	uint32_t runs = 1;
	for (uint32_t k = 1; k < zcount; k++) runs += clear[k] != clear[k - 1];
	if (runs > 8) std::fill(clear.begin(), clear.end(), (uint8_t)0);         /* (a geometry that alternates: one launch of the fallback) */
	for (uint32_t begin = 0, k = 1; k <= zcount; k++) {
		if (k < zcount && clear[k] == clear[begin]) continue;
		cut.emplace_back();
		DasDecision &d = cut.back();
		decide_das(pb, plan, tx, zfirst + begin, k - begin, clear[begin] ? mode : fallback_mode, d);
		if (!clear[begin] && (d.path == DasPath_Staged || d.path == DasPath_Tile)) {
			d = DasDecision{};                                                        /* (cannot happen: the general kernel) */
			decide_das(pb, plan, tx, zfirst + begin, k - begin, row_end_fallback_mode(mode, BeamformerHipDasPath_General), d);
		}
		d.row_end_fallback = !clear[begin];
		d.a.row_ends = d.general.row_ends = clear[begin] ? 0u : 1u;
		begin = k;
	}
	parts.swap(cut);
}

/* ---------------------------------------------------------------- the multi-frame routes, on single-frame decisions */

/* launches of the ingest and of every pre-DAS stage for frame_count RF frames of a plan: one, but the filters share a grid axis with
 * the channels and take the frames in chunks of bf_stage_frame_chunk (stages.hip) */
static uint32_t stage_launches(const Plan &plan, uint32_t frame_count)
{
	return (frame_count + bf_stage_frame_chunk(plan.channels) - 1) / bf_stage_frame_chunk(plan.channels);
}

/* single-frame DAS launches of a part list: one a part, none where the frame is only cleared */
static uint32_t single_launches(const std::vector<DasDecision> &parts)
{
	uint32_t n = 0;
	for (const DasDecision &d : parts) n += d.path != DasPath_Zero;
	return n;
}

/* One item (a view, a variant) of a push whose fused kernel takes items that run the general kernel in one part.  True: a candidate
 * for it; else the tally says what the item is instead -- cleared, cut by the row-end rule, on a faster kernel -- or nothing: another
 * family, or `no_kernel` (the push's flag against its fused kernel). */
struct ItemTally {
	uint32_t zero = 0, cut = 0, faster = 0;
	int      family = BF_DAS_RCA, faster_path = DasPath_General;      /* of the last item seen; of the last faster one */
};
static bool fused_candidate(const std::vector<DasDecision> &parts, bool no_kernel, ItemTally &t)
{
	const DasDecision &head = main_part(parts);
	t.family = head.a.family;
	if (head.path == DasPath_Zero) { t.zero++; return false; }
	if (parts.size() != 1) { t.cut++; return false; }
	if (head.path != DasPath_General) { t.faster++; t.faster_path = head.path; return false; }
	return head.a.family == BF_DAS_RCA && !no_kernel;
}

void decide_burst(const ParameterBlock &pb, const Plan &plan, const std::vector<BfTransmit> &tx, const std::vector<DasDecision> &parts,
                  uint32_t zfirst, uint32_t zcount, uint32_t mode, uint32_t frame_count, BurstDecision &out, bool readi_sweep)
{
	out = BurstDecision{};
	out.readi_sweep = readi_sweep;
	out.stage_launches = stage_launches(plan, frame_count);
	if (parts.empty()) {                                 /* no DAS stage in the plan, or no planes: nothing was decided */
		out.min_frames = readi_sweep ? kReadiSweepMinFrames : kBurstMinFrames;
		out.single_path = -1;
		out.reason = "no DAS stage runs: the frames are cleared";
		return;
	}
	const DasDecision &head = main_part(parts);
	const bool sweep = readi_sweep && head.a.family == BF_DAS_READI;                  /* the family the sweep kernel exists for */
	const uint32_t min_frames = sweep ? kReadiSweepMinFrames : kBurstMinFrames;
	out.min_frames = min_frames;
	out.single_path = head.path;
	out.das_launches = single_launches(parts) * frame_count;
	char text[160];
	if (plan.das_index < 0 || zcount == 0) {
		out.reason = "no DAS stage runs: the frames are cleared";
	} else if (head.path == DasPath_Zero) {
		out.reason = "acquisition kind or interpolation mode the shader leaves at zero: the frames are cleared";
	} else if (mode & BeamformerHipDasPath_NoBurstKernel) {
		out.reason = "das path flag 0x400: the single-frame kernel once per frame was asked for";
	} else if (head.a.family != BF_DAS_RCA && !sweep) {
		out.reason = "the burst kernel exists for the RCA family (Flash, RCA_TPW, RCA_VLS) only: this family runs its single-frame kernel once per frame";
	} else if (parts.size() != 1) {
		out.reason = "the row-end rule cuts the frame into parts run by different kernels: the single-frame launches once per frame";
	} else if (head.path != DasPath_General) {
		std::snprintf(text, sizeof(text), "single frames run the %s, which already shares the geometry across its loops: it runs once per frame", das_path_name(head.path));
		out.reason = text;
	} else if (frame_count < min_frames) {
		std::snprintf(text, sizeof(text), "fewer than %u frames: the single-frame general kernel", min_frames);
		out.reason = text;
	} else {
		/* the general kernel's tiles at one thread per voxel: the frames fill the chip, not a channel split */
		DasDecision whole;
		decide_das(pb, plan, tx, zfirst, zcount, mode | BeamformerHipDasPath_NoChannelSplit, whole);
		out.a = whole.general;
		out.a.row_ends = head.general.row_ends;
		out.burst_kernel = true;
		out.frames_per_thread = BF_BURST_FRAMES_PER_THREAD;
		out.das_launches = 1;
		std::snprintf(text, sizeof(text), sweep ? "READI sweep on the general kernel: one launch, each thread applies a term's geometry to %u frames, each with its group's signs"
		                                        : "RCA family on the general kernel: one launch, each thread applies a term's geometry to %u frames", BF_BURST_FRAMES_PER_THREAD);
		out.reason = text;
	}
}

void derive_readi_image(const ParameterBlock &pb, const Plan &plan, ParameterBlock &derived_pb, Plan &derived_plan)
{
	derived_pb = pb;
	BeamformerParameters &bp = derived_pb.parameters;
	bp.acquisition_kind  = BeamformerAcquisitionKind_FORCES;
	bp.acquisition_count = pb.parameters.readi_group_count * pb.parameters.acquisition_count;
	bp.readi_group_count = 0; bp.readi_group = 0;
	derived_plan = plan;
	derived_plan.acquisitions = bp.acquisition_count;
	derived_plan.das_sparse = false;
	derived_plan.readi_hadamard.clear();
}

void decide_readi_image(const Plan &derived_plan, const std::vector<DasDecision> &parts, uint32_t group_count, uint32_t frame_count, ReadiImageDecision &out)
{
	out = ReadiImageDecision{};
	out.transmit_count = derived_plan.acquisitions;
	out.stage_launches = stage_launches(derived_plan, frame_count);
	if (parts.empty()) { out.reason = "no DAS stage runs: the frame is cleared"; return; }
	const DasDecision &head = main_part(parts);
	out.path = head.path;
	out.das_launches = single_launches(parts);
	char text[160];
	if (head.path == DasPath_Zero) {
		out.reason = "interpolation mode the shader leaves at zero: the frame is cleared";
	} else {
		out.decode_launches = 1;
		std::snprintf(text, sizeof(text), "READI image: %u acquisitions decoded across %u groups into %u FORCES transmits, one pass of the %s",
		              frame_count, group_count, out.transmit_count, das_path_name(head.path));
		out.reason = text;
	}
}

void plan_on_view(const ParameterBlock &pb, const ViewGrid &view, Plan &plan)
{
	const BeamformerParameters &bp = pb.parameters;
	for (int k = 0; k < 3; k++) plan.output_points[k] = view.points[k] > 1 ? view.points[k] : 1u;
	std::memcpy(plan.das_voxel_transform, view.transform, sizeof(plan.das_voxel_transform));
	if (bp.acquisition_kind == BeamformerAcquisitionKind_UFORCES || bp.acquisition_kind == BeamformerAcquisitionKind_FORCES)
		m4_mul(bp.xdc_transform, view.transform, plan.das_voxel_transform);
}

/* decide_views; any_tile_count: the eligible views are taken however few their tiles (what flag 0x1000 asks of a views push, and what a
 * burst views push's fused kernel does: there the frames fill the chip) */
static void decide_views_for(const ParameterBlock &pb, const Plan &plan, const std::vector<BfTransmit> &tx, const ViewGrid *views, uint32_t view_count,
                             uint32_t mode, bool any_tile_count, ViewsDecision &out)
{
	out = ViewsDecision{};
	out.parts.resize(view_count);
	out.taken.assign(view_count, 0);
	if (plan.das_index < 0) { out.reason = "no DAS stage runs: the frames are cleared"; return; }
	Plan on_view = plan;                         /* one copy; per view only the grid changes */
	std::vector<BfViewRow> rows(view_count);
	std::vector<uint8_t> eligible(view_count, 0);
	uint32_t tiles = 0, candidates = 0;
	const bool no_kernel = (mode & BeamformerHipDasPath_NoViewsKernel) != 0;
	ItemTally t;
	for (uint32_t v = 0; v < view_count; v++) {
		plan_on_view(pb, views[v], on_view);
		const uint32_t zcount = on_view.output_points[2];
		std::vector<DasDecision> &parts = out.parts[v];
		decide_das_parts(pb, on_view, tx, 0, zcount, mode, parts);
		out.das_launches += single_launches(parts);
		if (!fused_candidate(parts, no_kernel, t)) continue;
		const DasDecision &head = parts[0];
		/* the general kernel's tiles at one thread per voxel (decide_das under flag 0x10): the views fill the chip, not a channel split */
		BfViewRow &r = rows[v];
		r = BfViewRow{};
		BfDasArgs g = head.general;
		float to_xdc[16];
		voxel_to_xdc(g.family, pb, on_view, to_xdc);
		const int depth_axis = choose_tile(to_xdc, g.size, zcount, g.tile_shift, 8);
		uint32_t view_tiles = 1;
		for (int k = 0; k < 3; k++) {
			r.size[k] = g.size[k]; r.tile_shift[k] = g.tile_shift[k];
			r.blocks[k] = blocks_at(g.size[k], g.tile_shift[k]);
			view_tiles *= r.blocks[k];
		}
		r.depth_major = tile_walk(depth_axis, zcount, r.blocks[1], r.band_rows);
		if (r.depth_major == 3u) { r.depth_major = 2u; r.band_rows = 1; }      /* a view plane's balanced bands deal padded ids to the XCDs: here y fastest */
		std::memcpy(r.voxel_transform, on_view.das_voxel_transform, sizeof(r.voxel_transform));
		if ((uint64_t)tiles + view_tiles > 0x7FFFFFFFu) continue;               /* (grid x: such a view runs its own launch) */
		eligible[v] = 1; candidates++; tiles += view_tiles;
		out.a = head.general;                                                   /* (what is not the grid is the same in every view) */
	}
	char text[160];
	const bool take = candidates && (tiles >= kViewsMinTiles || any_tile_count);
	if (take) {
		uint32_t row_ends = 0, next = 0;
		for (uint32_t v = 0; v < view_count; v++) {
			if (!eligible[v]) continue;
			const DasDecision &head = out.parts[v][0];
			row_ends |= head.general.row_ends;
			out.taken[v] = 1;
			out.first_block.push_back(next);
			next += rows[v].blocks[0] * rows[v].blocks[1] * rows[v].blocks[2];
			out.rows.push_back(rows[v]);
			out.das_launches--;                                             /* its single-frame launch does not run */
		}
		out.first_block.push_back(next);
		out.kernel_views = candidates; out.kernel_tiles = tiles; out.das_launches++;
		out.a.split_shift = 0; out.a.row_ends = row_ends;
		std::snprintf(text, sizeof(text), "RCA family on the general kernel: %u of %u views, %u tiles, in one launch of the views kernel", candidates, view_count, tiles);
	} else if (t.zero == view_count) {
		std::snprintf(text, sizeof(text), "acquisition kind or interpolation mode the shader leaves at zero: the frames are cleared");
	} else if (no_kernel) {
		std::snprintf(text, sizeof(text), "das path flag 0x800: each view's single-frame kernel on the shared DAS input was asked for");
	} else if (t.family != BF_DAS_RCA) {
		std::snprintf(text, sizeof(text), "the views kernel exists for the RCA family (Flash, RCA_TPW, RCA_VLS) only: this family runs its single-frame kernel once per view");
	} else if (!candidates) {
		if (t.faster) std::snprintf(text, sizeof(text), "single frames on these grids run the %s: it runs once per view on the shared DAS input", das_path_name(t.faster_path));
		else if (t.cut) std::snprintf(text, sizeof(text), "the row-end rule cuts the views into parts run by different kernels: the single-frame launches once per view");
		else          std::snprintf(text, sizeof(text), "no view the views kernel can take: each runs its own launch");
	} else {
		std::snprintf(text, sizeof(text), "fewer than %u tiles in the eligible views: the single-frame general kernel once per view", kViewsMinTiles);
	}
	out.reason = text;
}

void decide_views(const ParameterBlock &pb, const Plan &plan, const std::vector<BfTransmit> &tx, const ViewGrid *views, uint32_t view_count,
                  uint32_t mode, ViewsDecision &out)
{
	decide_views_for(pb, plan, tx, views, view_count, mode, (mode & BeamformerHipDasPath_PreferViewsKernel) != 0, out);
}

void decide_burst_views(const ParameterBlock &pb, const Plan &plan, const std::vector<BfTransmit> &tx, const ViewGrid *views, uint32_t view_count,
                        uint32_t mode, uint32_t frame_count, BurstViewsDecision &out)
{
	out = BurstViewsDecision{};
	const uint32_t N = frame_count;
	out.stage_launches = stage_launches(plan, N);
	const bool per_frame_asked = (mode & BeamformerHipDasPath_NoBurstKernel) != 0;
	const bool fused_asked = N >= kBurstViewsMinFrames && !per_frame_asked && !(mode & BeamformerHipDasPath_NoViewsKernel);
	/* rung 1: the views the views kernel is eligible for, whatever their tile count; rungs 2 and 3: decide_views' own rules (under 0x800 it
	 * takes no view) */
	if (fused_asked) decide_views_for(pb, plan, tx, views, view_count, mode, true, out.views);
	else             decide_views(pb, plan, tx, views, view_count, mode, out.views);
	const ViewsDecision &v = out.views;
	uint32_t own = 0;                        /* single-frame launches of the views no kernel takes, for one RF frame */
	for (uint32_t k = 0; k < view_count; k++)
		if (!v.taken[k]) own += single_launches(v.parts[k]);
	char text[160];
	if (fused_asked && v.kernel_views) {
		out.rung = 1;
		out.kernel_views = v.kernel_views; out.frames_per_thread = BF_BURST_FRAMES_PER_THREAD;
		out.das_launches = 1 + N * own;
		if (v.kernel_views == view_count)
			std::snprintf(text, sizeof(text), "RCA family on the general kernel: %u views, %u tiles, %u frames in one launch, a term's geometry applied to %u frames",
			              v.kernel_views, v.kernel_tiles, N, BF_BURST_FRAMES_PER_THREAD);
		else
			std::snprintf(text, sizeof(text), "%u of %u views (%u tiles) x %u frames in one fused launch; the other views' single-frame launches once per RF frame: %u",
			              v.kernel_views, view_count, v.kernel_tiles, N, N * own);
		out.reason = text;
	} else if (v.kernel_views) {
		out.rung = 2;
		out.frame_kernel_views = v.kernel_views;
		out.das_launches = N * v.das_launches;
		if (per_frame_asked) std::snprintf(text, sizeof(text), "das path flag 0x400: the views kernel once per RF frame (%u of %u views) was asked for", v.kernel_views, view_count);
		else               std::snprintf(text, sizeof(text), "fewer than %u frames: the views kernel once per RF frame (%u of %u views)", kBurstViewsMinFrames, v.kernel_views, view_count);
		out.reason = text;
	} else {
		out.rung = 3;
		out.das_launches = N * v.das_launches;
		out.reason = v.reason.empty() ? std::string("each view's single-frame launch(es) once per RF frame") : v.reason + ", per RF frame";
	}
}

void derive_variant(const ParameterBlock &pb, const Plan &plan, const DasVariant &variant, ParameterBlock &derived_pb, Plan &derived_plan)
{
	derived_pb = pb;
	BeamformerParameters &bp = derived_pb.parameters;
	bp.speed_of_sound = variant.speed_of_sound;
	bp.time_offset    = variant.time_offset;
	bp.f_number       = variant.f_number;
	derived_plan = Plan{};
	derived_plan.stages = plan.stages;
	derived_plan.das_index = plan.das_index; derived_plan.iq_pipeline = plan.iq_pipeline; derived_plan.pipeline_data_kind = plan.pipeline_data_kind;
	derived_plan.channels = plan.channels; derived_plan.acquisitions = plan.acquisitions; derived_plan.raw_samples = plan.raw_samples;
	derived_plan.das_samples = plan.das_samples; derived_plan.das_sampling_frequency = plan.das_sampling_frequency;
	derived_plan.decimation = plan.decimation; derived_plan.das_sparse = plan.das_sparse;
	derived_plan.hadamard_base_order = plan.hadamard_base_order; derived_plan.intermediate_bytes = plan.intermediate_bytes;
	std::memcpy(derived_plan.output_points, plan.output_points, sizeof(plan.output_points));
	std::memcpy(derived_plan.das_voxel_transform, plan.das_voxel_transform, sizeof(plan.das_voxel_transform));
	/* planner.cpp: time_offset = bp.time_offset, then += every Filter / Demodulate / Hilbert stage's delay on the way to DAS */
	float time_offset = variant.time_offset;
	for (int i = 0; i < plan.das_index && i < (int)plan.stages.size(); i++) {
		const Stage &st = plan.stages[(size_t)i];
		if (st.kind == BeamformerShaderKind_Filter || st.kind == BeamformerShaderKind_Demodulate || st.kind == BeamformerShaderKind_Hilbert)
			time_offset += st.filter.time_delay;
	}
	derived_plan.das_time_offset = time_offset;
}

void decide_variants(const ParameterBlock &pb, const Plan &plan, const std::vector<BfTransmit> &tx, const DasVariant *variants, uint32_t variant_count,
                     uint32_t mode, VariantsDecision &out, const std::vector<DasDecision> *const *known)
{
	out = VariantsDecision{};
	out.parts.resize(variant_count);
	out.taken.assign(variant_count, 0);
	if (plan.das_index < 0) { out.reason = "no DAS stage runs: the frames are cleared"; return; }
	const uint32_t zcount = plan.output_points[2];
	std::vector<uint8_t> eligible(variant_count, 0);
	uint32_t candidates = 0;
	const bool no_kernel = (mode & BeamformerHipDasPath_NoVariantsKernel) != 0;
	ItemTally t;
	ParameterBlock derived_pb;
	Plan derived_plan;
	for (uint32_t v = 0; v < variant_count; v++) {
		std::vector<DasDecision> &parts = out.parts[v];
		if (known && known[v]) {
			parts = *known[v];
		} else {
			derive_variant(pb, plan, variants[v], derived_pb, derived_plan);
			decide_das_parts(derived_pb, derived_plan, tx, 0, zcount, mode, parts);
		}
		out.das_launches += single_launches(parts);
		if (!fused_candidate(parts, no_kernel, t)) continue;
		eligible[v] = 1; candidates++;
	}
	/* the general kernel's tiles at one thread per voxel (decide_das under flag 0x10), the same for every variant: the grid is the block's */
	uint64_t tiles = 0;
	if (candidates) {
		DasDecision whole;
		decide_das(pb, plan, tx, 0, zcount, mode | BeamformerHipDasPath_NoChannelSplit, whole);
		out.a = whole.general;
		if (out.a.depth_major == 3u) { out.a.depth_major = 2u; out.a.band_rows = 1; }      /* a view plane's balanced bands deal padded ids to the XCDs: here y fastest */
		tiles = (uint64_t)out.a.blocks[0] * out.a.blocks[1] * out.a.blocks[2];
		if (tiles == 0 || tiles > 0x7FFFFFFFu) candidates = 0;                            /* (grid x: such a grid runs its own launches) */
	}
	char text[160];
	const bool take = candidates && (tiles * candidates >= kVariantsMinTiles || candidates >= kVariantsMinVariants || (mode & BeamformerHipDasPath_PreferVariantsKernel));
	if (take) {
		uint32_t row_ends = 0;
		for (uint32_t v = 0; v < variant_count; v++) {
			if (!eligible[v]) continue;
			const BfDasArgs &g = out.parts[v][0].general;      /* the five fields as decide_das fills them for the derived block */
			BfVariantRow r{};
			r.speed_of_sound = g.speed_of_sound; r.inv_speed_of_sound = g.inv_speed_of_sound;
			r.time_offset = g.time_offset; r.f_number = g.f_number; r.edge_margin = g.edge_margin;
			if (out.rows.empty()) {
				out.a.speed_of_sound = g.speed_of_sound; out.a.inv_speed_of_sound = g.inv_speed_of_sound;
				out.a.time_offset = g.time_offset; out.a.f_number = g.f_number; out.a.edge_margin = g.edge_margin;
			}
			row_ends |= g.row_ends;
			out.taken[v] = 1;
			out.rows.push_back(r);
			out.das_launches--;                                                 /* its single-frame launch does not run */
		}
		out.kernel_variants = candidates; out.kernel_tiles = (uint32_t)(tiles * candidates > 0xFFFFFFFFull ? 0xFFFFFFFFull : tiles * candidates);
		out.das_launches++;
		out.a.split_shift = 0; out.a.row_ends = row_ends;
		out.a.z_first = 0; out.a.z_count = out.a.size[2];
		std::snprintf(text, sizeof(text), "RCA family on the general kernel: %u of %u variants x %u tiles in one launch of the variants kernel", candidates, variant_count, (uint32_t)tiles);
	} else if (t.zero == variant_count) {
		std::snprintf(text, sizeof(text), "acquisition kind or interpolation mode the shader leaves at zero: the frames are cleared");
	} else if (no_kernel) {
		std::snprintf(text, sizeof(text), "das path flag 0x4000: each variant's single-frame kernel on the shared DAS input was asked for");
	} else if (t.family != BF_DAS_RCA) {
		std::snprintf(text, sizeof(text), "the variants kernel exists for the RCA family (Flash, RCA_TPW, RCA_VLS) only: this family runs its single-frame kernel once per variant");
	} else if (!candidates) {
		if (t.faster) std::snprintf(text, sizeof(text), "single frames on this grid run the %s: it runs once per variant on the shared DAS input", das_path_name(t.faster_path));
		else if (t.cut) std::snprintf(text, sizeof(text), "the row-end rule cuts the frames into parts run by different kernels: the single-frame launches once per variant");
		else          std::snprintf(text, sizeof(text), "no variant the variants kernel can take: each runs its own launch");
	} else {
		std::snprintf(text, sizeof(text), "fewer than %u eligible variants and fewer than %u variants x tiles: the single-frame general kernel once per variant",
		              kVariantsMinVariants, kVariantsMinTiles);
	}
	out.reason = text;
}

uint32_t row_end_planes(const std::vector<DasDecision> &parts)
{
	uint32_t n = 0;
	for (const DasDecision &d : parts) if (d.row_end_fallback) n += d.z_count;
	return n;
}

const DasDecision &main_part(const std::vector<DasDecision> &parts)
{
	size_t best = 0;
	for (size_t i = 1; i < parts.size(); i++) if (parts[i].z_count > parts[best].z_count) best = i;
	return parts[best];
}

} // namespace bf
