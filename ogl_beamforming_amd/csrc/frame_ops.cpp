/* frame_ops.cpp -- the calls that work on frames already in the ring.  The reduce calls (score, quantiles, find_peaks, accumulate_peaks,
 * pair_peaks, track_peaks, draw_tracks, gram, gram_boxes, correlate) read the newest frames where they lie and end in a synchronise.
 * The two deposit maps -- the localisation map and the track map -- are what the peak calls add to.  The queued runs (mix, mix_field,
 * autocorrelate, convolve, warp, queue_localisation_map, queue_track_map) write frames of their own behind the newest ones and do not
 * synchronise.  Their device state is Device::ops (context.h: FrameOps); the ring -- ids, placement, records, timing slots -- is
 * executor.cpp's. */
#include "context.h"
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>

namespace bf {

void FrameOps::release()
{
	for (DeviceBuffer *b : {&metrics_scratch, &peaks_list, &map.buffer, &tracks.buffer, &tracks_scratch, &mix_table, &blend_table, &spatial_scratch}) b->release();
	for (void *p : {metrics_pinned, mix_pinned, blend_pinned}) if (p) (void)hipHostFree(p);
	for (hipEvent_t e : {metrics_begin, metrics_end, peaks_begin, peaks_end, mix_copied, mix_begin, mix_end, blend_copied}) if (e) (void)hipEventDestroy(e);
	*this = FrameOps{};
}

/* beamformer_hip_peak_threshold_of: the number to hand to the peak calls for a decision value -- the value itself for real frames; for
 * complex ones the largest float32 T >= 0 with fl(T * T) <= value.  The product is formed in float32 on its own, as the mark pass forms
 * it, and rounding is monotone: the condition holds up to one T and fails from the next, so the T is found by bisection over the bit
 * patterns of the non-negative floats -- what stepping from sqrtf(value) with nextafterf arrives at, without the 10^8 steps that takes
 * where the products underflow (value 0: every T up to 2^-75). */
float peak_threshold_of(float value, bool cplx)
{
	if (!cplx) return value;
	const auto holds = [value](uint32_t bits) {
		float t; std::memcpy(&t, &bits, sizeof(t));
		volatile float p = t * t;                          /* (one rounding to float32, whatever the host evaluates in) */
		return p <= value;
	};
	uint32_t lo = 0, hi = 0x7F7FFFFFu;                     /* holds(lo): 0 <= value; the largest finite float may hold too */
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo + 1u) / 2u;
		if (holds(mid)) lo = mid; else hi = mid - 1u;
	}
	float t; std::memcpy(&t, &lo, sizeof(t));
	return t;
}

namespace {

/* one of the `count` newest frames as score_last_frames and find_peaks_last_frames take it: its record, and the box inside it */
struct BoxedFrame {
	const FrameRecord *record;
	uint32_t first[3], count[3], cplx;
	uint64_t volume;                 /* voxels of the box */
};

/* The `count` newest frames of the one device, oldest first, each with the box of `region` (NULL: the frame whole).  The records are
 * judged the way export_last_frames and sum_last_frames judge theirs -- but ANY frame missing refuses: something per frame is promised.
 * False, with InvalidAccess set: no device or several, fewer frames queued, a tombstone, an overwritten record, reused storage, a box
 * that does not fit inside every frame, a frame that does not lie inside the ring. */
bool newest_boxed_frames(uint32_t count, const BeamformerHipFrameRegion *region, std::vector<BoxedFrame> &out)
{
	Context &c = ctx();
	/* several devices: a frame is a set of z-slabs there, and a z neighbour would lie across them */
	if (!c.device_ready || c.device_count != 1) return set_error(BeamformerLibErrorKind_InvalidAccess);
	Device &d = c.devices[0];
	if (count > d.frame_counter || count > d.frames.size()) return set_error(BeamformerLibErrorKind_InvalidAccess);
	if (region) for (int k = 0; k < 3; k++) if (!region->count[k]) return set_error(BeamformerLibErrorKind_InvalidAccess);
	out.resize(count);
	const uint64_t first_id = d.frame_counter - count;
	for (uint32_t n = 0; n < count; n++) {
		const FrameRecord &f = d.frames[(first_id + n) % d.frames.size()];
		if (f.id != (uint32_t)(first_id + n) || f.failed || !f.bytes) return set_error(BeamformerLibErrorKind_InvalidAccess);
		BoxedFrame &b = out[n];
		b.record = &f;
		b.cplx = f.data_kind == BeamformerDataKind_Float32Complex;
		b.volume = 1;
		for (int k = 0; k < 3; k++) {
			b.first[k] = region ? region->first[k] : 0u;
			b.count[k] = region ? region->count[k] : f.points[k];
			/* the box inside the frame (a frame of no voxels -- a pipeline without DAS on a peer -- holds no box) */
			if (!b.count[k] || (uint64_t)b.first[k] + b.count[k] > f.points[k]) return set_error(BeamformerLibErrorKind_InvalidAccess);
			b.volume *= b.count[k];     /* (at most the frame's voxels, which fit its record's 64-bit byte count) */
		}
		/* and the frame inside the ring: what the kernels index with is what the record says */
		if (f.offset > d.ring.size || f.bytes > d.ring.size - f.offset ||
		    (uint64_t)f.points[0] * f.points[1] * f.points[2] * (b.cplx ? 8u : 4u) > f.bytes) return set_error(BeamformerLibErrorKind_InvalidAccess);
	}
	return true;
}

/* the `count` newest frames as the ensemble calls take them: of one grid and one kind (else DataSizeMismatch), boxed */
bool newest_ensemble_frames(uint32_t count, const BeamformerHipFrameRegion *region, std::vector<BoxedFrame> &boxed)
{
	if (!newest_boxed_frames(count, region, boxed)) return false;
	const FrameRecord &f0 = *boxed[0].record;
	for (uint32_t n = 1; n < count; n++) {
		const FrameRecord &f = *boxed[n].record;
		if (f.data_kind != f0.data_kind || f.points[0] != f0.points[0] || f.points[1] != f0.points[1] || f.points[2] != f0.points[2])
			return set_error(BeamformerLibErrorKind_DataSizeMismatch);
	}
	return true;
}

/* a boxed frame's ABI record (BeamformerHipFrameMetrics, BeamformerHipFramePeaks, BeamformerHipMapDeposits): zeroed, and the fields the three begin with */
template <class M> void describe_frame(M &m, const BoxedFrame &b)
{
	const FrameRecord &f = *b.record;
	std::memset(&m, 0, sizeof(m));
	m.frame_id = f.id; m.parameter_block = f.block; m.data_kind = (uint32_t)f.data_kind; m.image_plane_tag = f.tag;
	for (int k = 0; k < 3; k++) { m.points[k] = f.points[k]; m.region_first[k] = b.first[k]; m.region_count[k] = b.count[k]; }
}

/* a boxed frame's kernel row (BfMetricsRow, BfPeaksRow): zeroed, and where the frame and its box lie */
template <class Row> void box_into(Row &r, const BoxedFrame &b)
{
	r = Row{}; r.offset = b.record->offset; r.cplx = b.cplx;
	for (int k = 0; k < 3; k++) { r.points[k] = b.record->points[k]; r.first[k] = b.first[k]; r.count[k] = b.count[k]; }
}

/* The tables of a reduce call, one behind the other, each from a 64-byte boundary: take() is a table's offset in the device scratch --
 * and in the pinned block, which holds the leading tables at the same offsets (its bytes: `total` once they are taken). */
struct Carve { size_t total = 0; size_t take(size_t bytes) { const size_t at = total; total += round_up(bytes, 64); return at; } };
/* ... and a table of `n` T taken from one: in(base) is the table in the block that starts at `base` -- the scratch, or the pinned block */
template <class T> struct Table {
	size_t at = 0;
	void take(Carve &c, size_t n) { at = c.take(sizeof(T) * n); }
	T *in(void *base) const { return (T *)((char *)base + at); }
};

/* the pinned memory, the device scratch and the first event pair the reduce calls share: each ends in a synchronise, so all is free again when it returns */
bool ensure_metrics_memory(Device &d, size_t pinned_bytes, size_t device_bytes)
{
	FrameOps &o = d.ops;
	bool ok = HIP_OK(hipSetDevice(d.device));
	if (ok && o.metrics_pinned_size < pinned_bytes) {
		if (o.metrics_pinned) (void)hipHostFree(o.metrics_pinned);
		o.metrics_pinned = nullptr; o.metrics_pinned_size = 0;
		ok = HIP_OK(hipHostMalloc(&o.metrics_pinned, pinned_bytes, hipHostMallocDefault));
		if (ok) o.metrics_pinned_size = pinned_bytes; else o.metrics_pinned = nullptr;
	}
	ok = ok && o.metrics_scratch.ensure(device_bytes);
	if (ok && !o.metrics_begin) ok = HIP_OK(hipEventCreate(&o.metrics_begin));
	if (ok && !o.metrics_end)   ok = HIP_OK(hipEventCreate(&o.metrics_end));
	return ok;
}

/* What a reduce call enqueues and waits for: the first up_bytes of the pinned block sent to the scratch, launch(stream) between the
 * metrics event pair, [down_at, down_at + down_bytes) of the scratch brought back to the same place in the pinned block.  The one
 * synchronise is also what frees the pinned memory for the next call, so it runs whatever failed before it.  False: InvalidAccess set.
 * also(stream): copies of the call's own to the caller's memory, enqueued behind the events and in front of the synchronise. */
template <class Launch, class Also> bool timed_reduce(Device &d, size_t up_bytes, size_t down_at, size_t down_bytes, float *device_ms, Launch launch, Also also)
{
	char *device = (char *)d.ops.metrics_scratch.ptr, *pinned = (char *)d.ops.metrics_pinned;
	hipStream_t s = d.stream;
	bool ok = HIP_OK(hipMemcpyAsync(device, pinned, up_bytes, hipMemcpyHostToDevice, s));
	ok &= HIP_OK(hipEventRecord(d.ops.metrics_begin, s));
	if (ok) ok &= HIP_OK(launch(s));
	ok &= HIP_OK(hipEventRecord(d.ops.metrics_end, s));
	if (ok) ok &= HIP_OK(hipMemcpyAsync(pinned + down_at, device + down_at, down_bytes, hipMemcpyDeviceToHost, s));
	if (ok) ok &= HIP_OK(also(s));
	ok &= HIP_OK(hipStreamSynchronize(s));
	if (!ok) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_InvalidAccess); }
	float ms = 0;
	if (device_ms) *device_ms = HIP_OK(hipEventElapsedTime(&ms, d.ops.metrics_begin, d.ops.metrics_end)) ? ms : 0.0f;
	return true;
}
template <class Launch> bool timed_reduce(Device &d, size_t up_bytes, size_t down_at, size_t down_bytes, float *device_ms, Launch launch)
{
	return timed_reduce(d, up_bytes, down_at, down_bytes, device_ms, launch, [](hipStream_t) { return hipSuccess; });
}

/* the mark pass's rows of the boxed frames (frame_peaks.hip): the waves and blocks of all frames, the most blocks of one.  False, with
 * InvalidAccess set: a box of more waves than the kernels number */
struct PeaksRows {
	std::vector<BfPeaksRow> rows;
	uint64_t waves = 0, blocks = 0;
	uint32_t max_blocks = 0;
};
bool peaks_rows_of(const std::vector<BoxedFrame> &boxed, const PeakQuery &q, PeaksRows &out)
{
	const uint32_t count = (uint32_t)boxed.size();
	out.rows.resize(count);
	for (uint32_t n = 0; n < count; n++) {
		const BoxedFrame &b = boxed[n];
		BfPeaksRow &r = out.rows[n];
		box_into(r, b);
		const uint64_t per_row = ((uint64_t)r.count[0] + 63u) / 64u, frame_waves = per_row * r.count[1] * r.count[2];
		/* (a frame of the ring has far fewer voxels than this: a bound that keeps the kernels' 32-bit wave numbers honest) */
		if (frame_waves > 4ull * BF_PEAKS_MAX_BLOCKS - 3u) return set_error(BeamformerLibErrorKind_InvalidAccess);
		r.waves_per_row = (uint32_t)per_row;
		r.waves = (uint32_t)frame_waves;
		r.blocks = (uint32_t)((frame_waves + 3u) / 4u);
		r.wave_first = out.waves; r.block_first = out.blocks;
		const float t = q.threshold_of(n);
		r.threshold = b.cplx ? t * t : t;
		r.cap = q.max_per_frame;                           /* (the emit pass's: a call without one leaves it 0) */
		out.waves += r.waves; out.blocks += r.blocks;
		if (r.blocks > out.max_blocks) out.max_blocks = r.blocks;
	}
	return true;
}

/* What the five peak calls do first (frame_peaks.hip: mark, scan): the rows of the boxed frames, the mark pass's tables carved from the
 * reduce calls' scratch, the rows -- and the placements, of a call that has them -- in pinned memory, the mark launch, and what the
 * scan found turned into the numbers that size everything behind it.  The caller fills `boxed` (newest_boxed_frames), decides its own
 * refusals, then prepare(); then run() -- the first synchronise --, or mark() inside a timed_reduce of its own.
 * device: rows | placements | results | lead | masks | counts | offsets | tail; pinned: up to the end of `lead` -- the tables of the
 * call's own that travel: rows and placements go up in one copy, what comes back starts at results. */
struct MarkFront {
	std::vector<BoxedFrame> boxed;
	PeaksRows table;
	uint32_t count = 0, cap = 0;
	Carve dev;
	size_t up_bytes = 0;
	Table<BfPeaksRow> rows; Table<double> placements; Table<BfPeaksResult> results; Table<uint64_t> masks; Table<uint32_t> counts, offsets;
	char *device = nullptr, *pinned = nullptr;
	/* what the scan found, from run() on: each frame's stored records and the first of them in the packed list, their number, and for the
	 * calls that link frames the most of one frame, the sum over the frame pairs of min(stored[n], stored[n + 1]) and the match pass's blocks */
	std::vector<uint32_t> stored, firsts, block_firsts;
	uint32_t total = 0, max_stored = 0, blocks = 0;                  /* (at most 1024 frames x 65536 records, 256 blocks a frame) */
	uint64_t capacity = 0;
	float mark_ms = 0;
	bool timed = false;

	/* lead(carve), tail(carve): the call takes its own tables there */
	template <class Lead, class Tail> bool prepare(Device &d, const PeakQuery &q, Lead lead, Tail tail)
	{
		count = (uint32_t)boxed.size(); cap = q.max_per_frame;
		if (!peaks_rows_of(boxed, q, table)) return false;
		const uint32_t placed = q.placements ? count : 0u;
		rows.take(dev, count); placements.take(dev, 12 * (size_t)placed); results.take(dev, count);
		up_bytes = placements.at + sizeof(double) * 12 * placed;
		lead(dev);
		const size_t pinned_bytes = dev.total;
		masks.take(dev, table.waves); counts.take(dev, table.blocks); offsets.take(dev, table.blocks);
		tail(dev);
		if (!ensure_metrics_memory(d, pinned_bytes, dev.total)) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_InvalidAccess); }
		device = (char *)d.ops.metrics_scratch.ptr; pinned = (char *)d.ops.metrics_pinned;
		std::memcpy(rows.in(pinned), table.rows.data(), sizeof(BfPeaksRow) * count);
		for (uint32_t n = 0; n < placed; n++) std::memcpy(placements.in(pinned) + 12 * (size_t)n, q.placement_of(n), sizeof(double) * 12);
		return true;
	}
	template <class Lead> bool prepare(Device &d, const PeakQuery &q, Lead lead) { return prepare(d, q, lead, [](Carve &) {}); }

	hipError_t mark(Device &d, hipStream_t s) const
	{
		return bf_launch_frame_peaks_mark(d.ring.ptr, rows.in(device), count, table.max_blocks, masks.in(device), counts.in(device), offsets.in(device),
		                                  results.in(device), s);
	}

	/* the mark pass on its own, for the calls whose buffers are sized by what it finds; its time is read here, with the rest's in device_ms() */
	bool run(Device &d)
	{
		bool ok = d.ops.peaks_begin || HIP_OK(hipEventCreate(&d.ops.peaks_begin));
		ok = ok && (d.ops.peaks_end || HIP_OK(hipEventCreate(&d.ops.peaks_end)));
		if (!ok) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_InvalidAccess); }
		if (!timed_reduce(d, up_bytes, results.at, sizeof(BfPeaksResult) * count, nullptr, [&](hipStream_t s) { return mark(d, s); })) return false;
		const BfPeaksResult *found = results.in(pinned);
		stored.resize(count); firsts.resize(count); block_firsts.resize(count - 1u);
		for (uint32_t n = 0; n < count; n++) {
			stored[n] = found[n].found < cap ? (uint32_t)found[n].found : cap;
			firsts[n] = total;
			total += stored[n];
			if (stored[n] > max_stored) max_stored = stored[n];
			if (n) capacity += stored[n - 1] < stored[n] ? stored[n - 1] : stored[n];
			if (n + 1u < count) { block_firsts[n] = blocks; blocks += (stored[n] + 255u) / 256u; }
		}
		timed = HIP_OK(hipEventElapsedTime(&mark_ms, d.ops.metrics_begin, d.ops.metrics_end));
		return true;
	}

	/* the call's device time: mark and scan, and -- `rest`: something was enqueued behind them, between the peaks event pair -- the rest */
	float device_ms(Device &d, bool rest) const
	{
		float rest_ms = 0;
		if (rest && !HIP_OK(hipEventElapsedTime(&rest_ms, d.ops.peaks_begin, d.ops.peaks_end))) rest_ms = 0;
		return timed ? mark_ms + rest_ms : 0.0f;
	}
};

/* What pair_peaks_last_frames, track_peaks_last_frames and draw_tracks_last_frames share behind the mark front: the peaks placed and
 * offered to one another (frame_peaks.hip: emit; frame_tracks.hip: place, nearest).  find() -- the first synchronise --, then the
 * caller takes its own tables from `big`, ensure(), enqueue(), its own launches, collect() -- the second.
 * lead: firsts | stored | block_firsts | unplaced | tallies | extra (the first three go up in one copy, unplaced, tallies and the
 * caller's `extra` come back in one: each group stays adjacent).  tracks_scratch: positions | forward | backward | the caller's. */
struct PeakChoices : MarkFront {
	uint32_t links = 0;
	Table<uint32_t> up_firsts, up_stored, up_block_firsts, unplaced;
	Table<BfTrackTally> tallies;
	Table<char> extra;
	size_t tally_bytes = 0;                                          /* from unplaced to the end of `extra` */
	Carve big;
	Table<double> positions;
	Table<uint32_t> forward, backward;
	char *scratch = nullptr;                                         /* tracks_scratch, from ensure() on */

	bool find(Device &d, const PeakQuery &q, size_t extra_bytes)
	{
		links = q.count - 1u;
		if (!prepare(d, q, [&](Carve &c) {
			up_firsts.take(c, q.count); up_stored.take(c, q.count); up_block_firsts.take(c, links); unplaced.take(c, q.count);
			tallies.take(c, links); extra.take(c, extra_bytes);
		}) || !run(d)) return false;
		tally_bytes = (extra_bytes ? extra.at + extra_bytes : tallies.at + sizeof(BfTrackTally) * links) - unplaced.at;
		std::memcpy(up_firsts.in(pinned), firsts.data(), sizeof(uint32_t) * count);
		std::memcpy(up_stored.in(pinned), stored.data(), sizeof(uint32_t) * count);
		std::memcpy(up_block_firsts.in(pinned), block_firsts.data(), sizeof(uint32_t) * links);
		std::memset(unplaced.in(pinned), 0, tally_bytes);
		positions.take(big, 3 * (size_t)total); forward.take(big, total); backward.take(big, total);
		return true;
	}

	bool ensure(Device &d)
	{
		const bool ok = d.ops.peaks_list.ensure((size_t)total * sizeof(BeamformerHipFramePeak)) && d.ops.tracks_scratch.ensure(big.total);
		scratch = (char *)d.ops.tracks_scratch.ptr;
		return ok;
	}

	/* behind ensure(), total != 0: the tables up, the tallies zeroed, the first event, then emit, place and -- with a frame pair that has
	 * peaks on both sides: else nothing is there to choose from -- nearest */
	bool enqueue(Device &d, const PeakQuery &q)
	{
		hipStream_t s = d.stream;
		const double reach = (double)q.max_distance;
		bool ok = HIP_OK(hipMemcpyAsync(up_firsts.in(device), up_firsts.in(pinned), unplaced.at - up_firsts.at, hipMemcpyHostToDevice, s));
		ok &= HIP_OK(hipMemsetAsync(unplaced.in(device), 0, tally_bytes, s));
		ok &= HIP_OK(hipEventRecord(d.ops.peaks_begin, s));
		if (ok) ok &= HIP_OK(bf_launch_frame_peaks_emit(d.ring.ptr, rows.in(device), count, table.max_blocks, masks.in(device), counts.in(device),
		                                                offsets.in(device), up_firsts.in(device), d.ops.peaks_list.ptr, s));
		if (ok) ok &= HIP_OK(bf_launch_tracks_place(d.ops.peaks_list.ptr, placements.in(device), up_firsts.in(device), up_stored.in(device), count,
		                                            max_stored, q.use_offsets != 0, positions.in(scratch), unplaced.in(device), s));
		if (ok && capacity) ok &= HIP_OK(bf_launch_tracks_nearest(positions.in(scratch), up_firsts.in(device), up_stored.in(device), count, max_stored,
		                                                          reach * reach, forward.in(scratch), backward.in(scratch), s));
		return ok;
	}

	/* the second event, the tallies back, the second synchronise -- which runs whatever failed before it */
	bool collect(Device &d, bool ok)
	{
		hipStream_t s = d.stream;
		ok &= HIP_OK(hipEventRecord(d.ops.peaks_end, s));
		if (ok) ok &= HIP_OK(hipMemcpyAsync(unplaced.in(pinned), unplaced.in(device), tally_bytes, hipMemcpyDeviceToHost, s));
		ok &= HIP_OK(hipStreamSynchronize(s));
		return ok;
	}
};

/* what a track or a draw call deposited, summed over its frames, and the maps its deposit bits name credited with it */
struct ChainDeposits {
	uint64_t points_deposited = 0, points_outside = 0, links = 0, links_deposited = 0, links_outside = 0;
	void credit(Device &d, uint32_t deposit, uint32_t block) const
	{
		if (deposit & BF_CHAIN_POINTS) d.ops.map.credit(block, 0, points_deposited, points_outside);
		if (deposit & BF_CHAIN_LINKS) d.ops.tracks.credit(block, links, links_deposited, links_outside);
	}
};

/* What track_peaks_last_frames and draw_tracks_last_frames share behind PeakChoices::find(), total != 0: the chain's tables carved from
 * tracks_scratch behind the choices -- next | links, twice | lengths | tails | track_of | first_of | words | offsets | tracks | points,
 * the two record lists sized by ALL stored records, an upper bound, or left out -- and the chain's launches behind enqueue(). */
struct ChainTables {
	Table<uint32_t> next, lengths, tails, track_of, first_of, words, offsets;
	Table<char> links, tracks, points;
	bool with_tracks = false, with_points = false;
	void carve(PeakChoices &c, bool keep_tracks, bool keep_points)
	{
		const size_t chain_blocks = ((size_t)c.total + 255u) / 256u;
		next.take(c.big, c.total); links.take(c.big, 4 * sizeof(uint32_t) * c.total); lengths.take(c.big, c.total); tails.take(c.big, c.total);
		track_of.take(c.big, c.total); first_of.take(c.big, c.total); words.take(c.big, 2 * chain_blocks); offsets.take(c.big, 2 * chain_blocks);
		tracks.take(c.big, keep_tracks ? sizeof(BeamformerHipPeakTrack) * (size_t)c.total : 0);
		points.take(c.big, keep_points ? sizeof(BeamformerHipTrackPoint) * (size_t)c.total : 0);
		with_tracks = keep_tracks; with_points = keep_points;
	}
	void *tracks_in(char *scratch) const { return with_tracks ? tracks.in(scratch) : nullptr; }
	void *points_in(char *scratch) const { return with_points ? points.in(scratch) : nullptr; }
	/* a: the maps' grids are filled in here, from the maps a.deposit names (the caller has checked that they exist) */
	hipError_t launch(Device &d, PeakChoices &c, BfChainArgs a, BfChainTally *tallies, hipStream_t s) const
	{
		const FrameOps::DepositMap &point_map = d.ops.map, &link_map = d.ops.tracks;
		const bool to_points = a.deposit & BF_CHAIN_POINTS, to_links = a.deposit & BF_CHAIN_LINKS;
		for (int k = 0; k < 3; k++) { a.point_map[k] = to_points ? point_map.points[k] : 0u; a.track_map[k] = to_links ? link_map.points[k] : 0u; }
		return bf_launch_tracks_chain(c.positions.in(c.scratch), c.up_firsts.in(c.device), c.up_stored.in(c.device), c.count, c.max_stored, c.total,
		                              c.capacity ? c.forward.in(c.scratch) : nullptr, c.capacity ? c.backward.in(c.scratch) : nullptr, next.in(c.scratch),
		                              links.in(c.scratch), lengths.in(c.scratch), tails.in(c.scratch), track_of.in(c.scratch), first_of.in(c.scratch),
		                              words.in(c.scratch), offsets.in(c.scratch), &a, to_points ? (uint32_t *)point_map.buffer.ptr : nullptr,
		                              to_links ? (uint32_t *)link_map.buffer.ptr : nullptr,
		                              to_links ? (char *)link_map.buffer.ptr + link_map.sums_at() : nullptr, tracks_in(c.scratch), points_in(c.scratch),
		                              tallies, s);
	}
};

/* the deposit bits of the track and the draw call against the maps that exist */
bool maps_for(Device &d, uint32_t deposit)
{
	if (((deposit & BF_CHAIN_POINTS) && !d.ops.map.exists()) || ((deposit & BF_CHAIN_LINKS) && !d.ops.tracks.exists()))
		return set_error(BeamformerLibErrorKind_InvalidAccess);
	return true;
}

/* the blocks of a strided reduce over a boxed frame (frame_metrics.hip, frame_quantiles.hip) and what a thread's stride of all their
 * threads is in the box's coordinates */
template <class Row> void stride_into(Row &r, const BoxedFrame &b)
{
	r.blocks = bf_metrics_blocks(b.volume);
	const uint64_t stride = (uint64_t)r.blocks * 256u, plane = (uint64_t)r.count[0] * r.count[1];
	r.step[0] = (uint32_t)(stride % r.count[0]);
	r.step[1] = (uint32_t)(stride / r.count[0] % r.count[1]);
	r.step[2] = (uint32_t)(stride / plane);
}

/* the Gram kernels' arguments for `count` frames of box `b` (ensemble.hip, ensemble_blocks.hip) */
BfGramArgs gram_args_of(const BoxedFrame &b, uint32_t count)
{
	BfGramArgs a{};
	a.frames = count; a.cplx = b.cplx;
	for (int k = 0; k < 3; k++) { a.points[k] = b.record->points[k]; a.first[k] = b.first[k]; a.count[k] = b.count[k]; }
	a.volume = (uint32_t)b.volume;
	a.words = (uint32_t)((b.volume + BF_GRAM_WORD - 1u) / BF_GRAM_WORD);
	a.chunk_words = bf_gram_chunk_words(a.volume, count);
	a.chunks = (a.words + a.chunk_words - 1u) / a.chunk_words;
	a.tiles = bf_gram_tiles(count); a.tile_pairs = bf_gram_tile_pairs(count);
	return a;
}

/* ... and the ABI record of one Gram matrix: the frames, the box, and the two counts its result {voxels, non_finite, gram} begins with */
void ensemble_info_of(BeamformerHipEnsembleInfo &info, const BfGramArgs &a, const FrameRecord &oldest, const char *result)
{
	std::memset(&info, 0, sizeof(info));
	info.count = a.frames; info.data_kind = (uint32_t)oldest.data_kind;
	for (int k = 0; k < 3; k++) { info.points[k] = a.points[k]; info.region_first[k] = a.first[k]; info.region_count[k] = a.count[k]; }
	info.first_frame_id = oldest.id;
	std::memcpy(&info.voxels, result, 8); std::memcpy(&info.non_finite, result + 8, 8);
}

/* The same `count` newest frames judged against each of `boxes` regions (regions null: one box, the frame whole), as the calls that
 * take a list of boxes need them: `frames` are the records, boxed by the first region, and row(r, box) hears of every box -- its oldest
 * frame stands for all: they are of one grid.  False, with the error set: what newest_ensemble_frames refuses, or a box of 2^32 voxels. */
template <class Each> bool frames_once_a_box(uint32_t count, const BeamformerHipFrameRegion *regions, uint32_t boxes, std::vector<BoxedFrame> &frames, Each row)
{
	std::vector<BoxedFrame> boxed;
	for (uint32_t r = 0; r < boxes; r++) {
		if (!newest_ensemble_frames(count, regions ? regions + r : nullptr, boxed)) return false;
		if (boxed[0].volume > 0xFFFFFFFFull) return set_error(BeamformerLibErrorKind_InvalidAccess);      /* the kernels count a box's voxels in 32 bits */
		if (r == 0) frames = boxed;
		row(r, boxed[0]);
	}
	return true;
}

} // namespace

/* beamformer_hip_score_last_frames: focus metrics of the `count` newest frames, reduced where they lie (frame_metrics.hip).  Everything
 * that can refuse is decided before anything is enqueued. */
bool score_last_frames(uint32_t count, const BeamformerHipFrameRegion *region, BeamformerHipFrameMetrics *out, float *device_ms)
{
	std::vector<BoxedFrame> boxed;
	if (!newest_boxed_frames(count, region, boxed)) return false;
	Device &d = ctx().devices[0];

	std::vector<BfMetricsRow> rows(count);
	uint32_t partials = 0, max_blocks = 0;
	for (uint32_t n = 0; n < count; n++) {
		BfMetricsRow &r = rows[n];
		box_into(r, boxed[n]);
		stride_into(r, boxed[n]);
		r.partial_first = partials;
		partials += r.blocks;
		if (r.blocks > max_blocks) max_blocks = r.blocks;
	}

	/* device: rows | results | partials; pinned: rows | results */
	Carve dev;
	const size_t rows_at = dev.take(sizeof(BfMetricsRow) * count), results_at = dev.take(sizeof(BfMetricsResult) * count), pinned_bytes = dev.total,
	             partials_at = dev.take(sizeof(BfMetricsPartial) * partials);
	if (!ensure_metrics_memory(d, pinned_bytes, dev.total)) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_InvalidAccess); }

	char *device = (char *)d.ops.metrics_scratch.ptr, *pinned = (char *)d.ops.metrics_pinned;
	const BfMetricsResult *results = (const BfMetricsResult *)(pinned + results_at);
	std::memcpy(pinned + rows_at, rows.data(), sizeof(BfMetricsRow) * count);
	if (!timed_reduce(d, sizeof(BfMetricsRow) * count, results_at, sizeof(BfMetricsResult) * count, device_ms, [&](hipStream_t s) {
		return bf_launch_frame_metrics(d.ring.ptr, (const BfMetricsRow *)(device + rows_at), count, max_blocks, (BfMetricsPartial *)(device + partials_at),
		                               (BfMetricsResult *)(device + results_at), s);
	})) return false;

	for (uint32_t n = 0; n < count; n++) {
		const FrameRecord &f = *boxed[n].record;
		const BfMetricsResult &v = results[n];
		BeamformerHipFrameMetrics &m = out[n];
		describe_frame(m, boxed[n]);
		const uint64_t plane = (uint64_t)f.points[0] * f.points[1];
		for (int k = 0; k < 3; k++) { m.gradient_pairs[k] = v.pairs[k]; m.gradient2[k] = v.g[k]; }
		m.max_index[0] = (uint32_t)(v.max_index % f.points[0]);
		m.max_index[1] = (uint32_t)(v.max_index / f.points[0] % f.points[1]);
		m.max_index[2] = (uint32_t)(v.max_index / plane);
		m.voxels = v.voxels; m.non_finite = v.bad;
		m.sum_abs = v.s1; m.sum_abs2 = v.s2; m.sum_abs4 = v.s4;
		m.max_abs = v.max_abs;
	}
	return true;
}

/* beamformer_hip_find_peaks_last_frames: the local maxima of the `count` newest frames, found where they lie (frame_peaks.hip).  The
 * arguments arrive checked (lib_api.cpp); everything else that can refuse is decided before anything is enqueued.  Two synchronises:
 * the list buffer is sized by what the scan found. */
bool find_peaks_last_frames(const PeakQuery &q, BeamformerHipFramePeaks *frames, BeamformerHipFramePeak *peaks, uint32_t *peak_count, float *device_ms)
{
	static_assert(sizeof(BeamformerHipFramePeak) == 32 && sizeof(BeamformerHipFramePeaks) == 80, "records without padding");
	MarkFront f;
	if (!newest_boxed_frames(q.count, q.region, f.boxed)) return false;
	Device &d = ctx().devices[0];
	Table<uint32_t> up_firsts;                       /* lead: firsts */
	if (!f.prepare(d, q, [&](Carve &c) { up_firsts.take(c, q.count); }) || !f.run(d)) return false;

	if (f.total) {
		hipStream_t s = d.stream;
		std::memcpy(up_firsts.in(f.pinned), f.firsts.data(), sizeof(uint32_t) * q.count);
		bool ok = d.ops.peaks_list.ensure((size_t)f.total * sizeof(BeamformerHipFramePeak));
		if (ok) {
			ok &= HIP_OK(hipMemcpyAsync(up_firsts.in(f.device), up_firsts.in(f.pinned), sizeof(uint32_t) * q.count, hipMemcpyHostToDevice, s));
			ok &= HIP_OK(hipEventRecord(d.ops.peaks_begin, s));
			if (ok) ok &= HIP_OK(bf_launch_frame_peaks_emit(d.ring.ptr, f.rows.in(f.device), q.count, f.table.max_blocks, f.masks.in(f.device),
			                                                f.counts.in(f.device), f.offsets.in(f.device), up_firsts.in(f.device), d.ops.peaks_list.ptr, s));
			ok &= HIP_OK(hipEventRecord(d.ops.peaks_end, s));
			if (ok) ok &= HIP_OK(hipMemcpyAsync(peaks, d.ops.peaks_list.ptr, (size_t)f.total * sizeof(BeamformerHipFramePeak), hipMemcpyDeviceToHost, s));
			ok &= HIP_OK(hipStreamSynchronize(s));
		}
		if (!ok) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_InvalidAccess); }
	}
	if (device_ms) *device_ms = f.device_ms(d, f.total != 0);

	const BfPeaksResult *results = f.results.in(f.pinned);
	for (uint32_t n = 0; n < q.count; n++) {
		BeamformerHipFramePeaks &m = frames[n];
		describe_frame(m, f.boxed[n]);
		m.threshold = q.threshold_of(n);
		m.first = f.firsts[n]; m.stored = f.stored[n];
		m.found = results[n].found; m.above_threshold = results[n].above_threshold;
	}
	*peak_count = f.total;
	return true;
}

/* beamformer_hip_quantiles_last_frames: exact order statistics of the `count` newest frames, selected where they lie
 * (frame_quantiles.hip: three count passes, a pick behind each).  The arguments arrive checked (lib_api.cpp); everything else that can
 * refuse is decided before anything is enqueued.  One synchronise: no buffer is sized by what was counted. */
bool quantiles_last_frames(uint32_t count, const BeamformerHipFrameRegion *region, const double *fractions, uint32_t fraction_count,
                           BeamformerHipFrameQuantiles *frames, BeamformerHipFrameQuantile *quantiles, uint32_t *histograms, float *device_ms)
{
	static_assert(sizeof(BeamformerHipFrameQuantile) == 48 && sizeof(BeamformerHipFrameQuantiles) == 80, "records without padding");
	static_assert(BF_QUANTILES_MAX == BEAMFORMER_HIP_MAX_QUANTILES && BF_QUANTILES_BINS1 == BEAMFORMER_HIP_QUANTILE_BINS, "one limit");
	std::vector<BoxedFrame> boxed;
	if (!newest_boxed_frames(count, region, boxed)) return false;
	Device &d = ctx().devices[0];

	std::vector<BfQuantilesRow> rows(count);
	uint32_t max_blocks = 0;
	for (uint32_t n = 0; n < count; n++) {
		if (boxed[n].volume > 0xFFFFFFFFull) return set_error(BeamformerLibErrorKind_InvalidAccess);     /* the kernels count a box's voxels in 32 bits */
		BfQuantilesRow &r = rows[n];
		box_into(r, boxed[n]);
		stride_into(r, boxed[n]);
		if (r.blocks > max_blocks) max_blocks = r.blocks;
	}

	/* device: rows | fractions | tallies | states | count tables | prefixes; pinned: the first four
	 * (rows and fractions go up in one copy, tallies and states come back in one: each pair stays adjacent) */
	const size_t ranks = (size_t)count * fraction_count;
	Carve dev;
	const size_t rows_at = dev.take(sizeof(BfQuantilesRow) * count), fractions_at = dev.take(sizeof(double) * fraction_count),
	             tallies_at = dev.take(sizeof(BfQuantilesTally) * count), states_at = dev.take(sizeof(BfQuantileState) * ranks), pinned_bytes = dev.total,
	             tables_at = dev.take(sizeof(uint32_t) * bf_quantiles_table_words(count, fraction_count)),
	             prefixes_at = dev.take(sizeof(BfQuantilesPrefixes) * count);
	if (!ensure_metrics_memory(d, pinned_bytes, dev.total)) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_InvalidAccess); }

	char *device = (char *)d.ops.metrics_scratch.ptr, *pinned = (char *)d.ops.metrics_pinned;
	uint32_t *device_tables = (uint32_t *)(device + tables_at);
	const BfQuantilesTally *tallies = (const BfQuantilesTally *)(pinned + tallies_at);
	const BfQuantileState  *states  = (const BfQuantileState *)(pinned + states_at);
	std::memcpy(pinned + rows_at, rows.data(), sizeof(BfQuantilesRow) * count);
	std::memcpy(pinned + fractions_at, fractions, sizeof(double) * fraction_count);
	if (!timed_reduce(d, fractions_at + sizeof(double) * fraction_count, tallies_at, states_at - tallies_at + sizeof(BfQuantileState) * ranks, device_ms,
	                  [&](hipStream_t s) {
		return bf_launch_frame_quantiles(d.ring.ptr, (const BfQuantilesRow *)(device + rows_at), (const double *)(device + fractions_at), count, fraction_count,
		                                 max_blocks, device_tables, (BfQuantilesPrefixes *)(device + prefixes_at), (BfQuantilesTally *)(device + tallies_at),
		                                 (BfQuantileState *)(device + states_at), s);
	}, [&](hipStream_t s) {
		/* the first pass's tables as they are: [count][2048], straight to the caller's memory */
		return histograms ? hipMemcpyAsync(histograms, device_tables + bf_quantiles_pass1_at(count), sizeof(uint32_t) * BF_QUANTILES_BINS1 * count,
		                                   hipMemcpyDeviceToHost, s) : hipSuccess;
	})) return false;

	for (uint32_t n = 0; n < count; n++) {
		BeamformerHipFrameQuantiles &m = frames[n];
		describe_frame(m, boxed[n]);
		m.first = n * fraction_count; m.stored = fraction_count;
		m.voxels = tallies[n].voxels; m.non_finite = tallies[n].non_finite;
		for (uint32_t k = 0; k < fraction_count; k++) {
			const BfQuantileState &st = states[(size_t)n * fraction_count + k];
			BeamformerHipFrameQuantile &q = quantiles[(size_t)n * fraction_count + k];
			std::memset(&q, 0, sizeof(q));
			q.fraction = fractions[k];
			q.rank = st.rank; q.below = st.below; q.equal = st.equal;
			std::memcpy(&q.value, &st.value_bits, sizeof(float));
			q.magnitude = boxed[n].cplx ? sqrtf(q.value) : q.value;
			q.threshold = m.voxels ? peak_threshold_of(q.value, boxed[n].cplx != 0) : 0.0f;      /* (no finite voxel: every number 0) */
		}
	}
	return true;
}

/* beamformer_hip_localisation_map_reset, beamformer_hip_track_map_reset: one of the two maps of the one device, (re)allocated and zeroed
 * on the current stream; points null: released.  The extents arrive checked (lib_api.cpp). */
bool deposit_map_reset(FrameOps::DepositMap &map, const uint32_t points[3])
{
	Context &c = ctx();
	Device &d = c.devices[0];
	if (!points) {
		if (c.device_ready && map.buffer.ptr) {
			bool ok = HIP_OK(hipSetDevice(d.device));
			ok = ok && HIP_OK(hipStreamSynchronize(d.stream));          /* a deposit or a conversion may still be reading it */
			if (!ok) (void)hipGetLastError();
			map.buffer.release();
		}
		map.forget();
		return true;
	}
	if (!c.device_ready || c.device_count != 1) return set_error(BeamformerLibErrorKind_InvalidAccess);
	FrameOps::DepositMap shape(map.sum_components);
	for (int k = 0; k < 3; k++) shape.points[k] = points[k];
	const size_t bytes = shape.bytes();
	bool ok = HIP_OK(hipSetDevice(d.device));
	/* (a buffer that has to grow is freed first: what is enqueued on it must have run) */
	if (ok && map.buffer.ptr && map.buffer.size < bytes) ok = HIP_OK(hipStreamSynchronize(d.stream));
	if (!ok) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_InvalidAccess); }
	map.forget();                       /* (also when the buffer cannot be had: no map then) */
	if (!map.buffer.ensure(bytes)) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_RFDataSizeOverflow); }
	for (int k = 0; k < 3; k++) map.points[k] = points[k];
	if (!HIP_OK(hipMemsetAsync(map.buffer.ptr, 0, bytes, d.stream))) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_InvalidAccess); }
	return true;
}

/* beamformer_hip_accumulate_peaks_last_frames: the peaks of the `count` newest frames binned into the localisation map where they lie
 * (frame_peaks.hip: the mark pass and the scan of find_peaks_last_frames, then the deposit and the scan again over its words).  The
 * arguments arrive checked (lib_api.cpp); everything else that can refuse is decided before anything is enqueued.  One synchronise:
 * no buffer is sized by what was found. */
bool accumulate_peaks_last_frames(const PeakQuery &q, BeamformerHipMapDeposits *frames, float *device_ms)
{
	static_assert(sizeof(BeamformerHipMapDeposits) == 96 && sizeof(BeamformerHipMapInfo) == 32, "records without padding");
	static_assert(BF_MAP_MAX_VOXELS == BEAMFORMER_HIP_MAX_MAP_VOXELS, "one limit");
	MarkFront f;
	if (!newest_boxed_frames(q.count, q.region, f.boxed)) return false;
	Device &d = ctx().devices[0];
	FrameOps::DepositMap &map = d.ops.map;
	if (!map.exists()) return set_error(BeamformerLibErrorKind_InvalidAccess);
	/* lead: the deposit's tallies, which come back with the results in one copy; tail: its words */
	Table<BfPeaksResult> tallies;
	Table<uint32_t> words;
	if (!f.prepare(d, q, [&](Carve &c) { tallies.take(c, q.count); }, [&](Carve &c) { words.take(c, f.table.blocks); })) return false;
	BfMapArgs a{};
	for (int k = 0; k < 3; k++) a.points[k] = map.points[k];
	a.use_offsets = q.use_offsets != 0;
	if (!timed_reduce(d, f.up_bytes, f.results.at, tallies.at - f.results.at + sizeof(BfPeaksResult) * q.count, device_ms, [&](hipStream_t s) {
		const hipError_t e = f.mark(d, s);
		if (e != hipSuccess) return e;
		return bf_launch_localisation_deposit(d.ring.ptr, f.rows.in(f.device), f.placements.in(f.device), q.count, f.table.max_blocks, f.masks.in(f.device),
		                                      f.counts.in(f.device), f.offsets.in(f.device), &a, (uint32_t *)map.buffer.ptr, words.in(f.device),
		                                      tallies.in(f.device), s);
	})) return false;

	const BfPeaksResult *results = f.results.in(f.pinned), *deposits = tallies.in(f.pinned);
	uint64_t deposited = 0, outside = 0;
	for (uint32_t n = 0; n < q.count; n++) {
		deposited += deposits[n].found; outside += deposits[n].above_threshold;
		if (!frames) continue;
		BeamformerHipMapDeposits &m = frames[n];
		describe_frame(m, f.boxed[n]);
		m.threshold = q.threshold_of(n);
		m.found = results[n].found; m.above_threshold = results[n].above_threshold;
		m.deposited = deposits[n].found; m.outside = deposits[n].above_threshold;
	}
	map.credit(f.boxed[q.count - 1].record->block, 0, deposited, outside);
	return true;
}

/* the counts of a map that exists, `voxels` of them, -- and `sums`, where it has any -- as they are, behind everything enqueued on the
 * current stream.  False, with the error set: no such map (InvalidAccess), less room than voxels (ExportSpaceOverflow) */
static bool deposit_map_copy(const FrameOps::DepositMap &map, uint32_t *counts, int64_t *sums, uint64_t out_count)
{
	Context &c = ctx();
	Device &d = c.devices[0];
	if (!c.device_ready || c.device_count != 1 || !map.exists()) return set_error(BeamformerLibErrorKind_InvalidAccess);
	const uint64_t voxels = map.voxels();
	if (out_count < voxels) return set_error(BeamformerLibErrorKind_ExportSpaceOverflow);
	bool ok = HIP_OK(hipSetDevice(d.device));
	ok = ok && HIP_OK(hipMemcpyAsync(counts, map.buffer.ptr, sizeof(uint32_t) * voxels, hipMemcpyDeviceToHost, d.stream));
	if (sums)
		ok = ok && HIP_OK(hipMemcpyAsync(sums, (const char *)map.buffer.ptr + map.sums_at(), map.sum_components * sizeof(int64_t) * voxels,
		                                 hipMemcpyDeviceToHost, d.stream));
	ok = ok && HIP_OK(hipStreamSynchronize(d.stream));
	if (!ok) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_InvalidAccess); }
	return true;
}

/* ... and what both ABI info records hold of it: the grid and the totals (pairs: the track map's alone) */
template <class Info> static void deposit_map_info(const FrameOps::DepositMap &map, Info *info)
{
	std::memset(info, 0, sizeof(*info));
	for (int k = 0; k < 3; k++) info->points[k] = map.points[k];
	info->calls = map.calls; info->deposited = map.deposited; info->outside = map.outside;
}

/* beamformer_hip_localisation_map_copy */
bool localisation_map_copy(uint32_t *out, uint64_t out_count, BeamformerHipMapInfo *info)
{
	const FrameOps::DepositMap &map = ctx().devices[0].ops.map;
	if (!deposit_map_copy(map, out, nullptr, out_count)) return false;
	if (info) deposit_map_info(map, info);
	return true;
}

/* beamformer_hip_pair_peaks_last_frames: the peaks of the `count` newest frames linked frame to frame where they lie (frame_peaks.hip:
 * the mark pass, the scan and the emit pass of find_peaks_last_frames; frame_tracks.hip: place, nearest, match, scan, emit).  The
 * arguments arrive checked (lib_api.cpp); everything else that can refuse is decided before anything is enqueued.  Three synchronises
 * at the most: the buffers are sized by what the scan found, and the copy of the records by the pairs that were made. */
bool pair_peaks_last_frames(const PeakQuery &q, uint32_t deposit, BeamformerHipPeakPairs *rows, BeamformerHipPeakPair *pairs, uint32_t *pair_count,
                            float *device_ms)
{
	static_assert(sizeof(BeamformerHipPeakPair) == 48 && sizeof(BeamformerHipPeakPairs) == 72 && sizeof(BeamformerHipTrackMapInfo) == 40, "records without padding");
	static_assert(BF_TRACK_MAX_VOXELS == BEAMFORMER_HIP_MAX_TRACK_MAP_VOXELS && BF_TRACK_MAX_PEAKS == BEAMFORMER_HIP_MAX_PEAKS_PER_FRAME &&
	              BF_TRACK_COMPONENTS == BEAMFORMER_HIP_TRACK_MAP_COMPONENTS, "one limit");
	PeakChoices c;
	if (!newest_boxed_frames(q.count, q.region, c.boxed)) return false;
	Device &d = ctx().devices[0];
	FrameOps::DepositMap &map = d.ops.tracks;
	if (deposit && !map.exists()) return set_error(BeamformerLibErrorKind_InvalidAccess);
	if (!c.find(d, q, 0)) return false;
	const BfTrackTally *tallies = c.tallies.in(c.pinned);
	uint64_t total_pairs = 0;
	if (c.total) {
		/* tracks_scratch, behind the choices: masks | words | offsets | pairs */
		Table<uint64_t> pair_masks;
		Table<uint32_t> words, pair_offsets;
		Table<BeamformerHipPeakPair> made;
		pair_masks.take(c.big, 4 * (size_t)c.blocks); words.take(c.big, c.blocks); pair_offsets.take(c.big, c.blocks);
		made.take(c.big, pairs ? (size_t)c.capacity : 0);
		hipStream_t s = d.stream;
		bool ok = c.ensure(d);
		if (ok) {
			void *device_pairs = pairs && c.capacity ? made.in(c.scratch) : nullptr;
			BfTrackArgs a{};
			for (int k = 0; k < 3; k++) a.points[k] = deposit ? map.points[k] : 0u;
			a.deposit = deposit != 0;
			ok = c.enqueue(d, q);
			/* (no frame pair with peaks on both sides: every tally stays 0) */
			if (ok && c.capacity) ok &= HIP_OK(bf_launch_tracks_pair(c.positions.in(c.scratch), c.up_firsts.in(c.device), c.up_stored.in(c.device),
			                                                         c.up_block_firsts.in(c.device), q.count, c.max_stored, c.blocks, c.forward.in(c.scratch),
			                                                         c.backward.in(c.scratch), pair_masks.in(c.scratch), words.in(c.scratch),
			                                                         pair_offsets.in(c.scratch), &a, (uint32_t *)map.buffer.ptr,
			                                                         deposit ? (char *)map.buffer.ptr + map.sums_at() : nullptr, device_pairs,
			                                                         c.tallies.in(c.device), s));
			ok = c.collect(d, ok);
			for (uint32_t n = 0; n < c.links && ok; n++) total_pairs += tallies[n].pairs;
			if (ok && pairs && total_pairs) {
				ok = total_pairs <= c.capacity;                           /* (what the kernels promise: the copy below relies on it) */
				ok = ok && HIP_OK(hipMemcpyAsync(pairs, device_pairs, (size_t)total_pairs * sizeof(BeamformerHipPeakPair), hipMemcpyDeviceToHost, s));
				ok &= HIP_OK(hipStreamSynchronize(s));
			}
		}
		if (!ok) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_InvalidAccess); }
	}
	if (device_ms) *device_ms = c.device_ms(d, c.total != 0);

	const BfPeaksResult *results = c.results.in(c.pinned);
	const uint32_t *unplaced = c.unplaced.in(c.pinned);
	uint32_t first = 0;
	uint64_t deposited = 0, outside = 0;
	for (uint32_t n = 0; n < c.links; n++) {
		BeamformerHipPeakPairs &m = rows[n];
		const BfTrackTally &t = tallies[n];
		std::memset(&m, 0, sizeof(m));
		for (uint32_t k = 0; k < 2; k++) {
			m.frame_id[k] = c.boxed[n + k].record->id;
			m.threshold[k] = q.threshold_of(n + k);
			m.peaks[k] = c.stored[n + k]; m.found[k] = results[n + k].found;
			m.unplaced[k] = unplaced[n + k];
			m.unpaired[k] = c.stored[n + k] - unplaced[n + k] - t.pairs;
		}
		m.first = first; m.pairs = t.pairs; m.deposited = t.deposited; m.outside = t.outside;
		first += t.pairs;
		deposited += t.deposited; outside += t.outside;
	}
	if (deposit) map.credit(c.boxed[q.count - 1].record->block, first, deposited, outside);
	*pair_count = first;
	return true;
}

/* beamformer_hip_track_peaks_last_frames: the pairs of the `count` newest frames chained into tracks, the tracks of at least min_length
 * peaks listed and deposited (frame_tracks.hip: link, jump, keep, scan, finish, behind the launches pair_peaks_last_frames shares with
 * this call -- its own match, scan and emit are not needed: the chains are read off the choices).  The arguments arrive checked
 * (lib_api.cpp); everything else that can refuse is decided before anything is enqueued.  Three synchronises at the most, for the pair
 * call's reasons: the buffers are sized by what the scan found -- the two record lists by ALL stored records, an upper bound --, and
 * the two downloads by the tallies. */
bool track_peaks_last_frames(const PeakQuery &q, uint32_t min_length, uint32_t deposit, BeamformerHipTrackedFrame *rows, BeamformerHipPeakTrack *tracks,
                             BeamformerHipTrackPoint *points, uint32_t *track_count, uint32_t *point_count, float *device_ms)
{
	static_assert(sizeof(BeamformerHipPeakTrack) == 48 && sizeof(BeamformerHipTrackPoint) == 40 && sizeof(BeamformerHipTrackedFrame) == 56, "records without padding");
	static_assert(BF_CHAIN_POINTS == BEAMFORMER_HIP_TRACK_DEPOSIT_POINTS && BF_CHAIN_LINKS == BEAMFORMER_HIP_TRACK_DEPOSIT_LINKS, "one pair of bits");
	const uint32_t count = q.count;
	PeakChoices c;
	if (!newest_boxed_frames(count, q.region, c.boxed)) return false;
	Device &d = ctx().devices[0];
	if (!maps_for(d, deposit)) return false;
	if (!c.find(d, q, sizeof(BfChainTally) * count)) return false;               /* extra: the chain's tallies */
	const BfChainTally *tallies = (const BfChainTally *)c.extra.in(c.pinned);
	uint64_t total_tracks = 0, total_points = 0;
	if (c.total) {
		ChainTables t;
		t.carve(c, tracks != nullptr, points != nullptr);
		hipStream_t s = d.stream;
		bool ok = c.ensure(d);
		if (ok) {
			BfChainArgs a{};
			a.deposit = deposit; a.min_length = min_length;
			ok = c.enqueue(d, q);
			if (ok) ok &= HIP_OK(t.launch(d, c, a, (BfChainTally *)c.extra.in(c.device), s));
			ok = c.collect(d, ok);
			for (uint32_t n = 0; n < count && ok; n++) { total_tracks += tallies[n].kept_heads; total_points += tallies[n].kept_points; }
			ok = ok && total_tracks <= c.total && total_points <= c.total;      /* (what the kernels promise: the copies below rely on it) */
			const bool tracks_back = tracks && total_tracks, points_back = points && total_points;
			if (ok && tracks_back)
				ok = HIP_OK(hipMemcpyAsync(tracks, t.tracks_in(c.scratch), (size_t)total_tracks * sizeof(BeamformerHipPeakTrack), hipMemcpyDeviceToHost, s));
			if (ok && points_back)
				ok = HIP_OK(hipMemcpyAsync(points, t.points_in(c.scratch), (size_t)total_points * sizeof(BeamformerHipTrackPoint), hipMemcpyDeviceToHost, s));
			if (tracks_back || points_back) ok &= HIP_OK(hipStreamSynchronize(s));
		}
		if (!ok) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_InvalidAccess); }
	}
	if (device_ms) *device_ms = c.device_ms(d, c.total != 0);

	const BfPeaksResult *results = c.results.in(c.pinned);
	const uint32_t *unplaced = c.unplaced.in(c.pinned);
	ChainDeposits sum;
	for (uint32_t n = 0; n < count; n++) {
		BeamformerHipTrackedFrame &m = rows[n];
		const BfChainTally &t = tallies[n];
		std::memset(&m, 0, sizeof(m));
		m.frame_id = c.boxed[n].record->id; m.threshold = q.threshold_of(n);
		m.peaks = c.stored[n]; m.unplaced = unplaced[n];
		m.heads = t.heads; m.kept_heads = t.kept_heads; m.kept_points = t.kept_points; m.kept_links = t.kept_links;
		m.points_deposited = t.points_deposited; m.points_outside = t.points_outside;
		m.links_deposited = t.links_deposited; m.links_outside = t.links_outside;
		m.found = results[n].found;
		sum.points_deposited += t.points_deposited; sum.points_outside += t.points_outside;
		sum.links += t.kept_links; sum.links_deposited += t.links_deposited; sum.links_outside += t.links_outside;
	}
	sum.credit(d, deposit, c.boxed[count - 1].record->block);
	*track_count = (uint32_t)total_tracks; *point_count = (uint32_t)total_points;
	return true;
}

/* beamformer_hip_draw_tracks_last_frames: the track call's kept tracks, smoothed along the track and drawn into both maps at map
 * resolution (frame_tracks.hip: smooth, draw, behind the chain's launches, which run without a deposit of their own).  The two record
 * lists stay on the device, where the draw pass reads them; nothing is sized by what was kept, so there are TWO synchronises: the
 * counts and the tallies.  The arguments arrive checked (lib_api.cpp); everything else that can refuse is decided before anything is
 * enqueued. */
bool draw_tracks_last_frames(const PeakQuery &q, uint32_t min_length, uint32_t smooth, uint32_t deposit, BeamformerHipDrawnFrame *rows, float *device_ms)
{
	static_assert(sizeof(BeamformerHipDrawnFrame) == 64, "a record without padding");
	static_assert(BF_DRAW_MAX_SMOOTH == BEAMFORMER_HIP_MAX_TRACK_SMOOTH && BF_DRAW_MAX_SAMPLES == BEAMFORMER_HIP_MAX_LINK_SAMPLES, "one limit");
	const uint32_t count = q.count;
	PeakChoices c;
	if (!newest_boxed_frames(count, q.region, c.boxed)) return false;
	Device &d = ctx().devices[0];
	const FrameOps::DepositMap &point_map = d.ops.map, &link_map = d.ops.tracks;
	const bool with_points = deposit & BF_CHAIN_POINTS, with_links = deposit & BF_CHAIN_LINKS;
	if (!maps_for(d, deposit)) return false;
	/* extra: the chain's tallies, then the draw pass's */
	if (!c.find(d, q, (sizeof(BfChainTally) + sizeof(BfDrawTally)) * count)) return false;
	const BfChainTally *chained = (const BfChainTally *)c.extra.in(c.pinned);
	const BfDrawTally *drawn = (const BfDrawTally *)(chained + count);
	if (c.total) {
		ChainTables t;
		t.carve(c, true, true);
		Table<double> smoothed;
		smoothed.take(c.big, smooth ? 3 * (size_t)c.total : 0);
		hipStream_t s = d.stream;
		bool ok = c.ensure(d);
		if (ok) {
			BfChainTally *device_chained = (BfChainTally *)c.extra.in(c.device);
			BfChainArgs a{};
			a.min_length = min_length;                                      /* (deposit 0: the finish pass lists, the draw pass deposits) */
			BfDrawArgs w{};
			for (int k = 0; k < 3; k++) { w.point_map[k] = with_points ? point_map.points[k] : 0u; w.track_map[k] = with_links ? link_map.points[k] : 0u; }
			w.deposit = deposit; w.smooth = smooth;
			ok = c.enqueue(d, q);
			if (ok) ok &= HIP_OK(t.launch(d, c, a, device_chained, s));
			if (ok) ok &= HIP_OK(bf_launch_tracks_draw(c.up_firsts.in(c.device), c.up_stored.in(c.device), count, c.max_stored, c.total, t.links.in(c.scratch),
			                                           t.lengths.in(c.scratch), t.track_of.in(c.scratch), t.first_of.in(c.scratch), t.words.in(c.scratch),
			                                           t.offsets.in(c.scratch), t.tracks_in(c.scratch), t.points_in(c.scratch),
			                                           smooth ? smoothed.in(c.scratch) : nullptr, &w,
			                                           with_points ? (uint32_t *)point_map.buffer.ptr : nullptr,
			                                           with_links ? (uint32_t *)link_map.buffer.ptr : nullptr,
			                                           with_links ? (char *)link_map.buffer.ptr + link_map.sums_at() : nullptr,
			                                           (BfDrawTally *)(device_chained + count), s));
			ok = c.collect(d, ok);
		}
		if (!ok) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_InvalidAccess); }
	}
	if (device_ms) *device_ms = c.device_ms(d, c.total != 0);

	const BfPeaksResult *results = c.results.in(c.pinned);
	const uint32_t *unplaced = c.unplaced.in(c.pinned);
	ChainDeposits sum;
	for (uint32_t n = 0; n < count; n++) {
		BeamformerHipDrawnFrame &m = rows[n];
		const BfDrawTally &t = drawn[n];
		std::memset(&m, 0, sizeof(m));
		m.frame_id = c.boxed[n].record->id; m.threshold = q.threshold_of(n);
		m.peaks = c.stored[n]; m.unplaced = unplaced[n];
		m.kept_points = chained[n].kept_points; m.kept_links = chained[n].kept_links;
		m.lone = t.lone; m.links_skipped = t.links_skipped; m.samples = t.samples; m.repeats = t.repeats;
		m.points_deposited = t.points_deposited; m.points_outside = t.points_outside;
		m.links_deposited = t.links_deposited; m.links_outside = t.links_outside;
		m.found = results[n].found;
		sum.points_deposited += t.points_deposited; sum.points_outside += t.points_outside;
		sum.links += t.samples - t.repeats; sum.links_deposited += t.links_deposited; sum.links_outside += t.links_outside;
	}
	sum.credit(d, deposit, c.boxed[count - 1].record->block);
	return true;
}

/* beamformer_hip_track_map_copy */
bool track_map_copy(uint32_t *counts, int64_t *sums, uint64_t out_count, BeamformerHipTrackMapInfo *info)
{
	const FrameOps::DepositMap &map = ctx().devices[0].ops.tracks;
	if (!deposit_map_copy(map, counts, sums, out_count)) return false;
	if (info) { deposit_map_info(map, info); info->pairs = map.pairs; }
	return true;
}

/* beamformer_hip_gram_last_frames: the slow-time Gram matrix of the `count` newest frames, reduced where they lie (ensemble.hip).
 * Everything that can refuse is decided before anything is enqueued. */
bool gram_last_frames(uint32_t count, const BeamformerHipFrameRegion *region, double *gram, BeamformerHipEnsembleInfo *info, float *device_ms)
{
	static_assert(sizeof(BeamformerHipEnsembleInfo) == 64, "a record without padding");
	static_assert(BF_ENSEMBLE_MAX_FRAMES == BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES, "one limit");
	std::vector<BoxedFrame> boxed;
	if (!newest_ensemble_frames(count, region, boxed)) return false;
	Device &d = ctx().devices[0];
	const BoxedFrame &b0 = boxed[0];
	if (b0.volume > 0xFFFFFFFFull) return set_error(BeamformerLibErrorKind_InvalidAccess);     /* the kernels count a box's voxels in 32 bits */

	const BfGramArgs a = gram_args_of(b0, count);

	/* device: offsets | result {voxels, non_finite, gram} | mask | partials; pinned: offsets | result */
	const size_t gram_bytes = sizeof(double) * 2 * count * count;
	Carve dev;
	const size_t offsets_at = dev.take(sizeof(uint64_t) * count), result_at = dev.take(16 + gram_bytes), pinned_bytes = dev.total,
	             mask_at = dev.take(sizeof(uint64_t) * a.words), partials_at = dev.take(sizeof(double) * 2 * BF_GRAM_TILE * BF_GRAM_TILE * a.tile_pairs * a.chunks);
	if (!ensure_metrics_memory(d, pinned_bytes, dev.total)) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_InvalidAccess); }

	char *device = (char *)d.ops.metrics_scratch.ptr, *pinned = (char *)d.ops.metrics_pinned;
	uint64_t *offsets = (uint64_t *)(pinned + offsets_at);
	for (uint32_t n = 0; n < count; n++) offsets[n] = boxed[n].record->offset;
	const char *result = pinned + result_at;
	if (!timed_reduce(d, sizeof(uint64_t) * count, result_at, 16 + gram_bytes, device_ms, [&](hipStream_t s) {
		return bf_launch_gram(d.ring.ptr, (const uint64_t *)(device + offsets_at), &a, (uint64_t *)(device + mask_at), (double *)(device + partials_at),
		                      device + result_at, s);
	})) return false;
	std::memcpy(gram, result + 16, gram_bytes);
	if (info) ensemble_info_of(*info, a, *b0.record, result);
	return true;
}

namespace { uint64_t g_gram_boxes_budget = BF_BLOCKS_BUDGET; }
void set_gram_boxes_budget(uint64_t bytes) { g_gram_boxes_budget = bytes ? bytes : BF_BLOCKS_BUDGET; }

/* beamformer_hip_gram_boxes_last_frames: the Gram matrix of every box of a list, each what gram_last_frames gives for that box
 * (ensemble_blocks.hip).  The boxes are walked in BATCHES whose partials fit the budget (a box that does not fit one on its own is a batch
 * of one); a batch is one triple of launches, the batches sit behind one another on the stream and share one mask and one partials
 * buffer.  One upload (the frames' offsets and every box's row), one copy back (every box's result), one synchronise.  The counts arrive
 * checked (lib_api.cpp); everything else that can refuse is decided before anything is enqueued. */
bool gram_boxes_last_frames(uint32_t count, const BeamformerHipFrameRegion *regions, uint32_t region_count, double *grams,
                            BeamformerHipEnsembleInfo *infos, float *device_ms)
{
	static_assert(BF_BLOCKS_MAX_BOXES == BEAMFORMER_HIP_MAX_GRAM_BOXES, "one limit");
	struct Batch { uint32_t first, boxes, mask_blocks, partial_blocks; uint64_t mask_words, partial_tiles; };
	const uint64_t tile_bytes = sizeof(double) * 2 * BF_GRAM_TILE * BF_GRAM_TILE;
	const size_t gram_bytes = sizeof(double) * 2 * count * count, result_bytes = 16 + gram_bytes;

	std::vector<BoxedFrame> frames;
	std::vector<BfBlocksBox> rows(region_count);
	std::vector<Batch> batches;
	if (!frames_once_a_box(count, regions, region_count, frames, [&](uint32_t r, const BoxedFrame &b) {
		BfBlocksBox &row = rows[r];
		row = BfBlocksBox{};
		const BfGramArgs &a = row.a = gram_args_of(b, count);
		const uint64_t mask_blocks = (a.words + 3u) / 4u, partial_tiles = (uint64_t)a.chunks * a.tile_pairs;
		if (batches.empty() || (batches.back().partial_tiles + partial_tiles) * tile_bytes > g_gram_boxes_budget ||
		    batches.back().mask_blocks + mask_blocks > 0x7FFFFFFFull || batches.back().partial_blocks + partial_tiles > 0x7FFFFFFFull)
			batches.push_back(Batch{r, 0, 0, 0, 0, 0});
		Batch &batch = batches.back();
		row.mask_block_first = batch.mask_blocks; row.partial_block_first = batch.partial_blocks;
		row.mask_first = batch.mask_words; row.partial_first = batch.partial_tiles;
		row.result_first = (uint64_t)r * result_bytes;
		batch.boxes++; batch.mask_blocks += (uint32_t)mask_blocks; batch.partial_blocks += (uint32_t)partial_tiles;
		batch.mask_words += a.words; batch.partial_tiles += partial_tiles;
	})) return false;
	Device &d = ctx().devices[0];
	uint64_t mask_words = 0, partial_tiles = 0;
	for (const Batch &batch : batches) {
		if (batch.mask_words > mask_words) mask_words = batch.mask_words;
		if (batch.partial_tiles > partial_tiles) partial_tiles = batch.partial_tiles;
	}

	/* device: offsets | rows | results | mask | partials; pinned: offsets | rows | results */
	Carve dev;
	const size_t offsets_at = dev.take(sizeof(uint64_t) * count), rows_at = dev.take(sizeof(BfBlocksBox) * region_count),
	             results_at = dev.take(result_bytes * region_count), pinned_bytes = dev.total,
	             mask_at = dev.take(sizeof(uint64_t) * mask_words), partials_at = dev.take(tile_bytes * partial_tiles);
	if (!ensure_metrics_memory(d, pinned_bytes, dev.total)) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_InvalidAccess); }

	char *device = (char *)d.ops.metrics_scratch.ptr, *pinned = (char *)d.ops.metrics_pinned;
	uint64_t *offsets = (uint64_t *)(pinned + offsets_at);
	for (uint32_t n = 0; n < count; n++) offsets[n] = frames[n].record->offset;
	std::memcpy(pinned + rows_at, rows.data(), sizeof(BfBlocksBox) * region_count);
	if (!timed_reduce(d, rows_at + sizeof(BfBlocksBox) * region_count, results_at, result_bytes * region_count, device_ms, [&](hipStream_t s) {
		for (const Batch &batch : batches) {
			const hipError_t e = bf_launch_gram_boxes(d.ring.ptr, (const uint64_t *)(device + offsets_at), rows.data() + batch.first,
			                                          (const BfBlocksBox *)(device + rows_at) + batch.first, batch.boxes, batch.mask_blocks,
			                                          batch.partial_blocks, (uint64_t *)(device + mask_at), (double *)(device + partials_at),
			                                          device + results_at, s);
			if (e != hipSuccess) return e;
		}
		return hipSuccess;
	})) return false;
	for (uint32_t r = 0; r < region_count; r++) {
		const char *result = pinned + results_at + (size_t)r * result_bytes;
		std::memcpy((char *)grams + (size_t)r * gram_bytes, result + 16, gram_bytes);
		if (infos) ensemble_info_of(infos[r], rows[r].a, *frames[0].record, result);
	}
	return true;
}

/* beamformer_hip_correlate_last_frames: the `count` newest frames correlated with one of them at every shift of the window, over every
 * box, where they lie (correlate.hip).  The arguments arrive checked (lib_api.cpp: the counts, the window, the entry cap); everything
 * else that can refuse is decided before anything is enqueued. */
bool correlate_last_frames(uint32_t count, uint32_t reference, const BeamformerHipFrameRegion *regions, uint32_t region_count,
                           const uint32_t max_shift[3], BeamformerHipShiftCorrelation *table, BeamformerHipCorrelationInfo *info, float *device_ms)
{
	static_assert(sizeof(BeamformerHipShiftCorrelation) == 40 && sizeof(BfCorrelateEntry) == 40, "one record, without padding");
	static_assert(sizeof(BeamformerHipCorrelationInfo) == 56, "a record without padding");
	static_assert(BF_CORRELATE_MAX_SHIFT == BEAMFORMER_HIP_MAX_SHIFT && BF_CORRELATE_MAX_SHIFTS == BEAMFORMER_HIP_MAX_SHIFTS, "one limit");
	const uint32_t boxes = regions ? region_count : 1u;

	BfCorrelateArgs a{};
	a.frames = count; a.reference = reference; a.regions = boxes;
	a.shifts = 1;
	for (int k = 0; k < 3; k++) { a.max_shift[k] = max_shift[k]; a.window[k] = 2u * max_shift[k] + 1u; a.shifts *= a.window[k]; }
	a.groups = bf_correlate_groups(a.shifts);
	a.batches = (a.shifts + BF_CORRELATE_THREADS - 1u) / BF_CORRELATE_THREADS;

	std::vector<BoxedFrame> frames;
	std::vector<BfCorrelateRow> rows(boxes);
	uint64_t partials = 0;
	if (!frames_once_a_box(count, regions, boxes, frames, [&](uint32_t r, const BoxedFrame &b) {
		BfCorrelateRow &row = rows[r];
		row = BfCorrelateRow{};
		for (int k = 0; k < 3; k++) { row.first[k] = b.first[k]; row.count[k] = b.count[k]; }
		bf_correlate_tile(row.count, a.max_shift, row.tile);
		uint32_t tiles = 1;                                   /* (at most the box's voxels) */
		row.tile_voxels = 1; row.halo_voxels = 1;
		for (int k = 0; k < 3; k++) {
			row.tiles[k] = (row.count[k] + row.tile[k] - 1u) / row.tile[k];
			row.halo[k] = row.tile[k] + 2u * a.max_shift[k];
			tiles *= row.tiles[k]; row.tile_voxels *= row.tile[k]; row.halo_voxels *= row.halo[k];
		}
		row.chunk_tiles = bf_correlate_chunk_tiles(tiles, a.shifts);
		row.chunks = (tiles + row.chunk_tiles - 1u) / row.chunk_tiles;
		row.partial_first = partials;
		partials += (uint64_t)row.chunks * count * a.shifts;
		if (row.chunks > a.max_chunks) a.max_chunks = row.chunks;
	})) return false;
	Device &d = ctx().devices[0];
	const BoxedFrame &b0 = frames[0];
	a.cplx = b0.cplx;
	for (int k = 0; k < 3; k++) a.points[k] = b0.record->points[k];

	/* device: offsets | rows | table | partials; pinned: offsets | rows | table */
	const size_t entries = (size_t)boxes * count * a.shifts;
	Carve dev;
	const size_t offsets_at = dev.take(sizeof(uint64_t) * count), rows_at = dev.take(sizeof(BfCorrelateRow) * boxes),
	             table_at = dev.take(sizeof(BfCorrelateEntry) * entries), pinned_bytes = dev.total, partials_at = dev.take(sizeof(BfCorrelateEntry) * (size_t)partials);
	if (!ensure_metrics_memory(d, pinned_bytes, dev.total)) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_InvalidAccess); }

	char *device = (char *)d.ops.metrics_scratch.ptr, *pinned = (char *)d.ops.metrics_pinned;
	uint64_t *offsets = (uint64_t *)(pinned + offsets_at);
	for (uint32_t n = 0; n < count; n++) offsets[n] = frames[n].record->offset;
	std::memcpy(pinned + rows_at, rows.data(), sizeof(BfCorrelateRow) * boxes);
	if (!timed_reduce(d, rows_at + sizeof(BfCorrelateRow) * boxes, table_at, sizeof(BfCorrelateEntry) * entries, device_ms, [&](hipStream_t s) {
		return bf_launch_correlate(d.ring.ptr, (const uint64_t *)(device + offsets_at), (const BfCorrelateRow *)(device + rows_at), &a,
		                           (BfCorrelateEntry *)(device + partials_at), (BfCorrelateEntry *)(device + table_at), s);
	})) return false;
	std::memcpy(table, pinned + table_at, sizeof(BfCorrelateEntry) * entries);
	if (info) {
		std::memset(info, 0, sizeof(*info));
		info->count = count; info->reference = reference; info->data_kind = (uint32_t)b0.record->data_kind; info->region_count = boxes;
		for (int k = 0; k < 3; k++) { info->points[k] = a.points[k]; info->max_shift[k] = a.max_shift[k]; }
		info->shifts = a.shifts;
		info->first_frame_id = b0.record->id; info->reference_frame_id = frames[reference].record->id;
	}
	return true;
}

namespace {

/* What beamformer_hip_mix_last_frames, beamformer_hip_autocorrelate_last_frames, beamformer_hip_convolve_last_frames and
 * beamformer_hip_warp_last_frames share:
 * `out_count` frames computed from the `count` newest ones and queued as frames of their own behind them (and what
 * beamformer_hip_queue_localisation_map takes of it: a run without sources, RunTable::shape).  Everything that can refuse
 * is decided, and every buffer grown, before the ids are taken; nothing synchronises unless device_ms is asked for.
 * The call's table travels with the sources' ring offsets: a weight table of `rows` rows, laid out [tile][k][BF_MIX_TILE][2] (rows past
 * `rows` zero), or `flat_floats` floats as they are (the taps of a convolution), or neither (weights and flat null: the launch reads the
 * sources as they are).
 * prepare(device, newest source's record, cplx, out_count): what the call's launches need besides -- memory of their own --, grown
 * while the call can still refuse; false refuses it (InvalidAccess) with nothing changed.
 * launch(run): the call's kernel launches, one or several, on run.s -- the sources' offsets and the table in device memory (table null
 * without one), output j at ring + out_offset + j * out_stride. */
struct RunTable {
	const float *weights = nullptr; uint32_t rows = 0;
	const float *flat = nullptr;    uint32_t flat_floats = 0;
	/* true: `weights` holds `rows` rows that are judged as a mix's are (no imaginary part on real frames) but travel in a table of the
	 * call's own, which prepare() fills and launch() sends (beamformer_hip_mix_field_last_frames: a table a node) */
	bool own_table = false;
	/* not null: a run that has no source frames (count 0: beamformer_hip_queue_localisation_map) -- Float32 frames of this record's grid,
	 * carrying its block, stand where the newest source's record does */
	const FrameRecord *shape = nullptr;
};
struct QueuedRun {
	Device *d;
	void *ring;
	const uint64_t *offsets;
	const float *table;
	uint32_t K;
	bool cplx;
	uint32_t points[3];
	uint64_t elements, out_offset, out_stride;
	hipStream_t s;
};
const auto nothing_to_prepare = [](Device &, const FrameRecord &, bool, uint32_t) { return true; };

template <class Prepare, class Launch>
bool queue_frames_of_newest(uint32_t count, const RunTable &t, uint32_t out_count, uint32_t image_plane_tag,
                            uint32_t *first_frame_id, float *device_ms, Prepare prepare, Launch launch)
{
	const float *weights = t.weights;
	const uint32_t rows = t.rows;
	Context &c = ctx();
	std::vector<BoxedFrame> boxed;
	if (t.shape) {
		if (!c.device_ready || c.device_count != 1 || count != 0) return set_error(BeamformerLibErrorKind_InvalidAccess);
	} else if (!newest_ensemble_frames(count, nullptr, boxed)) return false;
	Device &d = c.devices[0];
	const FrameRecord newest = t.shape ? *t.shape : *boxed[count - 1].record;      /* (a copy: the run's records may take its place) */
	const bool cplx = t.shape ? false : boxed[0].cplx;
	if (!cplx && weights)
		for (size_t n = 0; n < (size_t)rows * count; n++)
			if (weights[2 * n + 1] != 0.0f) return set_error(BeamformerLibErrorKind_InvalidAccess);

	/* where the ring's placement rule will put the run, and whether that reuses storage of a source frame */
	const uint32_t K = count, M = out_count;
	uint64_t run_first = 0, run_bytes = 0;
	if (!queued_run_landing(d, newest.points, M, cplx, run_first, run_bytes)) return set_error(BeamformerLibErrorKind_FrameSizeOverflow);
	for (const BoxedFrame &b : boxed)
		if (b.record->offset < run_first + run_bytes && run_first < b.record->offset + b.record->bytes) return set_error(BeamformerLibErrorKind_FrameSizeOverflow);

	/* the table: offsets[K] | weights[tile][k][BF_MIX_TILE][2], rows past `rows` zero */
	const uint32_t padded = weights && !t.own_table ? (rows + BF_MIX_TILE - 1u) / BF_MIX_TILE * BF_MIX_TILE : 0u;
	const size_t offsets_bytes = round_up(sizeof(uint64_t) * K, 64), weights_bytes = t.flat ? sizeof(float) * t.flat_floats : sizeof(float) * 2 * padded * K;
	const size_t table_max = round_up(sizeof(uint64_t) * BF_ENSEMBLE_MAX_FRAMES, 64) + sizeof(float) * 2 * BF_ENSEMBLE_MAX_FRAMES * BF_ENSEMBLE_MAX_FRAMES;
	bool ok = HIP_OK(hipSetDevice(d.device));
	ok = ok && d.ops.mix_table.ensure(table_max);
	if (ok && !d.ops.mix_pinned && !HIP_OK(hipHostMalloc(&d.ops.mix_pinned, table_max, hipHostMallocDefault))) { d.ops.mix_pinned = nullptr; ok = false; }
	if (ok && !d.ops.mix_copied) ok = HIP_OK(hipEventCreateWithFlags(&d.ops.mix_copied, hipEventDisableTiming));
	if (ok && !d.ops.mix_begin)  ok = HIP_OK(hipEventCreate(&d.ops.mix_begin));
	if (ok && !d.ops.mix_end)    ok = HIP_OK(hipEventCreate(&d.ops.mix_end));
	ok = ok && weights_bytes <= table_max - offsets_bytes && prepare(d, newest, cplx, M);
	if (!ok) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_InvalidAccess); }
	if (d.ops.mix_copy_pending) { (void)hipEventSynchronize(d.ops.mix_copied); d.ops.mix_copy_pending = false; }   /* (the previous call's copy: long done) */
	char *pinned = (char *)d.ops.mix_pinned;
	uint64_t *offsets = (uint64_t *)pinned;
	for (uint32_t n = 0; n < K; n++) offsets[n] = boxed[n].record->offset;
	float *table = (float *)(pinned + offsets_bytes);
	std::memset(table, 0, weights_bytes);
	if (t.flat) std::memcpy(table, t.flat, weights_bytes);
	for (uint32_t j = 0; j < rows && weights && !t.own_table; j++)
		for (uint32_t k = 0; k < K; k++) {
			float *w = table + (((size_t)(j / BF_MIX_TILE) * K + k) * BF_MIX_TILE + j % BF_MIX_TILE) * 2;
			w[0] = weights[((size_t)j * K + k) * 2]; w[1] = weights[((size_t)j * K + k) * 2 + 1];
		}

	/* ---- from here on the call owns ids first .. first + M - 1, taken from the counters a push advances (claim_queued_run) ---- */
	return claim_queued_run(d, newest.points, image_plane_tag, M, cplx, newest.block, [&](uint64_t first, const FrameRecord &frame0) {
		hipStream_t s = d.stream;
		QueuedRun run{};
		run.d = &d; run.ring = d.ring.ptr; run.offsets = (const uint64_t *)d.ops.mix_table.ptr;
		run.table = (weights && !t.own_table) || t.flat ? (const float *)((const char *)d.ops.mix_table.ptr + offsets_bytes) : nullptr;
		run.K = K; run.cplx = cplx;
		for (int k = 0; k < 3; k++) run.points[k] = newest.points[k];
		run.elements = (uint64_t)newest.points[0] * newest.points[1] * newest.points[2];
		run.out_offset = frame0.offset; run.out_stride = frame0.bytes; run.s = s;
		if (offsets_bytes + weights_bytes) ok &= HIP_OK(hipMemcpyAsync(d.ops.mix_table.ptr, pinned, offsets_bytes + weights_bytes, hipMemcpyHostToDevice, s));
		d.ops.mix_copy_pending = HIP_OK(hipEventRecord(d.ops.mix_copied, s));
		ok &= d.ops.mix_copy_pending;
		if (device_ms) ok &= HIP_OK(hipEventRecord(d.ops.mix_begin, s));
		if (ok) ok &= HIP_OK(launch(run));
		if (device_ms) {
			ok &= HIP_OK(hipEventRecord(d.ops.mix_end, s));
			ok &= HIP_OK(hipStreamSynchronize(s));
			float ms = 0;
			if (ok) *device_ms = HIP_OK(hipEventElapsedTime(&ms, d.ops.mix_begin, d.ops.mix_end)) ? ms : 0.0f;
		}
		if (!ok) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_InvalidAccess); }
		if (first_frame_id) *first_frame_id = (uint32_t)first;
		return true;
	});
}

} // namespace

/* beamformer_hip_mix_last_frames: out_count linear combinations of the `count` newest frames, queued as frames of their own
 * (ensemble.hip) */
bool mix_last_frames(uint32_t count, const float *weights, uint32_t out_count, uint32_t image_plane_tag, uint32_t *first_frame_id, float *device_ms)
{
	RunTable t; t.weights = weights; t.rows = out_count;
	return queue_frames_of_newest(count, t, out_count, image_plane_tag, first_frame_id, device_ms, nothing_to_prepare,
		[=](const QueuedRun &r) {
			BfMixArgs a{};
			a.frames = r.K; a.outputs = out_count; a.cplx = r.cplx; a.padded_outputs = (out_count + BF_MIX_TILE - 1u) / BF_MIX_TILE * BF_MIX_TILE;
			a.elements = r.elements; a.out_offset = r.out_offset; a.out_stride = r.out_stride;
			return bf_launch_mix(r.ring, r.offsets, r.table, &a, r.s);
		});
}

/* which shape of the field mix runs where both apply -- a lattice without nodes along y --, by measurement (tools/block_filter_rate.py,
 * profiles/block_filter_rate.json) */
constexpr bool kBlendSourcesOnce = false;
namespace { int g_blend_shape = -1; }
void set_blend_shape(int shape) { g_blend_shape = shape; }

/* beamformer_hip_mix_field_last_frames: out_count combinations of the `count` newest frames under a weight table that varies over the
 * frame -- given at the nodes of a lattice, blended between them --, queued as frames of their own (ensemble_blocks.hip).  One launch.
 * The frame is cut into segment cells here: along axis a the segments [0, P_0), [P_j, P_j+1) and [P_N-1, points), each clipped to the
 * frame and left out when empty (one segment, the whole axis, where N_a == 1); a cell is the product of one segment an axis, and carries
 * its lower nodes, whether it blends along each axis, and the prefix of block counts the kernel finds its cell by.  The nodes' tables
 * -- each laid out as a mix's, [tile][k][BF_MIX_TILE][2], rows past out_count zero -- and the cells travel through pinned memory of the
 * call's own (FrameOps::blend_pinned), the sources' offsets through the skeleton's table. */
bool mix_field_last_frames(uint32_t count, const float *weights, const uint32_t nodes[3], const uint32_t node_first[3],
                           const uint32_t node_step[3], uint32_t out_count, uint32_t image_plane_tag, uint32_t *first_frame_id, float *device_ms)
{
	static_assert(BF_BLEND_MAX_NODES == BEAMFORMER_HIP_MAX_MIX_NODES && BF_BLEND_MAX_ENTRIES == BEAMFORMER_HIP_MAX_MIX_FIELD_ENTRIES, "one limit");
	const uint32_t node_product = nodes[0] * nodes[1] * nodes[2];
	const uint32_t K = count, M = out_count, padded = (M + BF_MIX_TILE - 1u) / BF_MIX_TILE * BF_MIX_TILE, tiles = padded / BF_MIX_TILE;
	const size_t node_floats = (size_t)2 * padded * K, weights_bytes = round_up(sizeof(float) * node_floats * node_product, 64);
	BfBlendArgs a{};
	a.frames = K; a.outputs = M; a.padded_outputs = padded;
	for (int k = 0; k < 3; k++) {
		a.nodes[k] = nodes[k];
		if (nodes[k] > 1u) a.inv_step[k] = 1.0f / (float)node_step[k];
	}
	/* the kernel's shape (ensemble_blocks.hip; the bytes are the same): hook BLEND_SHAPE, else kBlendSourcesOnce; sources-once has no lerp along y */
	a.once = (g_blend_shape < 0 ? kBlendSourcesOnce : g_blend_shape == 1) && nodes[1] == 1u;
	std::vector<BfBlendCell> cells;
	RunTable t; t.weights = weights; t.rows = node_product * M; t.own_table = true;
	return queue_frames_of_newest(count, t, out_count, image_plane_tag, first_frame_id, device_ms,
		[&](Device &d, const FrameRecord &newest, bool, uint32_t) {
			if ((uint64_t)newest.points[0] * newest.points[1] * newest.points[2] > 0x7FFFFFFFull) return false;   /* the kernel counts a cell's voxels in 32 bits */
			/* the segments of every axis: {first voxel, voxels, lower node, corners} */
			struct Segment { uint32_t first, count, node, corners; };
			std::vector<Segment> segments[3];
			for (int k = 0; k < 3; k++) {
				const uint64_t points = newest.points[k];
				if (nodes[k] == 1u) { segments[k].push_back(Segment{0u, (uint32_t)points, 0u, 1u}); continue; }
				const auto node_at = [&](uint32_t j) { const uint64_t at = (uint64_t)node_first[k] + (uint64_t)j * node_step[k]; return at < points ? at : points; };
				if (node_at(0) > 0) segments[k].push_back(Segment{0u, (uint32_t)node_at(0), 0u, 1u});
				for (uint32_t j = 0; j + 1u < nodes[k]; j++)
					if (node_at(j + 1u) > node_at(j)) segments[k].push_back(Segment{(uint32_t)node_at(j), (uint32_t)(node_at(j + 1u) - node_at(j)), j, 2u});
				if (node_at(nodes[k] - 1u) < points)
					segments[k].push_back(Segment{(uint32_t)node_at(nodes[k] - 1u), (uint32_t)(points - node_at(nodes[k] - 1u)), nodes[k] - 1u, 1u});
			}
			cells.clear();
			uint64_t blocks = 0;
			for (const Segment &sz : segments[2]) for (const Segment &sy : segments[1]) for (const Segment &sx : segments[0]) {
				const Segment *of[3] = {&sx, &sy, &sz};
				BfBlendCell cell{};
				cell.volume = 1;
				for (int k = 0; k < 3; k++) {
					cell.first[k] = of[k]->first; cell.count[k] = of[k]->count; cell.node[k] = of[k]->node; cell.corners[k] = of[k]->corners;
					cell.volume *= of[k]->count;
				}
				cell.block_first = (uint32_t)blocks;
				blocks += (uint64_t)((cell.volume + 255u) / 256u) * tiles;      /* (at most the frame's voxels x 16 tiles: below 2^35) */
				cells.push_back(cell);
			}
			if (blocks > 0x7FFFFFFFull) return false;
			a.cells = (uint32_t)cells.size(); a.blocks = (uint32_t)blocks;
			for (int k = 0; k < 3; k++) a.points[k] = newest.points[k];

			/* the call's own table: weights[node][tile][k][BF_MIX_TILE][2] | cells */
			FrameOps &o = d.ops;
			const size_t bytes = weights_bytes + sizeof(BfBlendCell) * cells.size();
			if (!o.blend_table.ensure(bytes)) return false;
			if (o.blend_copy_pending) { (void)hipEventSynchronize(o.blend_copied); o.blend_copy_pending = false; }   /* (the previous call's copy: long done) */
			if (o.blend_pinned_size < bytes) {
				if (o.blend_pinned) (void)hipHostFree(o.blend_pinned);
				o.blend_pinned = nullptr; o.blend_pinned_size = 0;
				if (!HIP_OK(hipHostMalloc(&o.blend_pinned, bytes, hipHostMallocDefault))) { o.blend_pinned = nullptr; return false; }
				o.blend_pinned_size = bytes;
			}
			if (!o.blend_copied && !HIP_OK(hipEventCreateWithFlags(&o.blend_copied, hipEventDisableTiming))) { o.blend_copied = nullptr; return false; }
			float *table = (float *)o.blend_pinned;
			std::memset(table, 0, weights_bytes);
			for (uint32_t c = 0; c < node_product; c++)
				for (uint32_t j = 0; j < M; j++)
					for (uint32_t k = 0; k < K; k++) {
						const float *from = weights + (((size_t)c * M + j) * K + k) * 2;
						float *w = table + (size_t)c * node_floats + (((size_t)(j / BF_MIX_TILE) * K + k) * BF_MIX_TILE + j % BF_MIX_TILE) * 2;
						w[0] = from[0]; w[1] = from[1];
					}
			std::memcpy((char *)o.blend_pinned + weights_bytes, cells.data(), sizeof(BfBlendCell) * cells.size());
			/* sent from here, in front of the event pair: nothing refuses the call any more, and the table is read by this call's launch alone */
			if (!HIP_OK(hipMemcpyAsync(o.blend_table.ptr, o.blend_pinned, bytes, hipMemcpyHostToDevice, d.stream))) return false;
			o.blend_copy_pending = HIP_OK(hipEventRecord(o.blend_copied, d.stream));
			return o.blend_copy_pending;
		},
		[&](const QueuedRun &r) {
			FrameOps &o = r.d->ops;
			BfBlendArgs args = a;
			args.cplx = r.cplx; args.out_offset = r.out_offset; args.out_stride = r.out_stride;
			return bf_launch_blend(r.ring, r.offsets, (const float *)o.blend_table.ptr, (const BfBlendCell *)((const char *)o.blend_table.ptr + weights_bytes),
			                       &args, r.s);
		});
}

/* beamformer_hip_autocorrelate_last_frames: lags 0 .. lag_count - 1 of the slow-time autocorrelation of `rows` mixes of the `count`
 * newest frames (weights null: of those frames themselves), queued as lag_count frames of their own (autocorr.hip) */
bool autocorrelate_last_frames(uint32_t count, const float *weights, uint32_t rows, uint32_t lag_count, uint32_t image_plane_tag,
                               uint32_t *first_frame_id, float *device_ms)
{
	static_assert(BF_AUTOCORR_MAX_LAGS == BEAMFORMER_HIP_MAX_LAGS, "one limit");
	RunTable t; t.weights = weights; t.rows = rows;
	return queue_frames_of_newest(count, t, lag_count, image_plane_tag, first_frame_id, device_ms, nothing_to_prepare,
		[=](const QueuedRun &r) {
			BfAutocorrArgs a{};
			a.frames = r.K; a.rows = rows; a.lags = lag_count; a.cplx = r.cplx;
			a.elements = r.elements; a.out_offset = r.out_offset; a.out_stride = r.out_stride;
			return bf_launch_autocorr(r.ring, r.offsets, r.table, &a, r.s);
		});
}

/* beamformer_hip_convolve_last_frames: the `count` newest frames filtered along x, y, z, queued as `count` frames of their own
 * (spatial.hip).  One launch a live axis.  P passes write, from the last one back, the output run, the scratch run, the output run: the
 * last pass writes the ring, and what lies between two passes is the library's own buffer or the run being made -- never a frame that
 * exists.  Scratch: one run's bytes when there are two passes or more, and in Normalised mode a D field (one float a voxel a frame) per
 * pass but the last, two at the most. */
bool convolve_last_frames(uint32_t count, const float *const taps[3], const uint32_t tap_counts[3], uint32_t mode, uint32_t image_plane_tag,
                          uint32_t *first_frame_id, float *device_ms)
{
	static_assert(BF_SPATIAL_MAX_TAPS == BEAMFORMER_HIP_MAX_SPATIAL_TAPS, "one limit");
	float table[3 * BF_SPATIAL_TAP_STRIDE] = {};                  /* an axis's row: zeros, the taps from BF_SPATIAL_TAP_FRONT on, zeros */
	uint32_t axes[3], passes = 0;
	for (uint32_t a = 0; a < 3; a++) {
		if (tap_counts[a] == 0) continue;
		axes[passes++] = a;
		std::memcpy(table + a * BF_SPATIAL_TAP_STRIDE + BF_SPATIAL_TAP_FRONT, taps[a], sizeof(float) * tap_counts[a]);
	}
	const uint32_t n[3] = {tap_counts[0], tap_counts[1], tap_counts[2]};
	const bool normalised = mode == BeamformerHipSpatialMode_Normalised;
	const uint32_t d_fields = normalised ? (passes - 1u < 2u ? passes - 1u : 2u) : 0u;
	const auto bytes_of = [](const FrameRecord &f, bool cplx, uint32_t frames, uint64_t &run, uint64_t &field) {
		const uint64_t voxels = (uint64_t)f.points[0] * f.points[1] * f.points[2];
		run = round_up(voxels * (cplx ? 8u : 4u), 64) * frames;
		field = round_up(voxels * 4u, 64) * frames;
	};
	RunTable t; t.flat = table; t.flat_floats = 3 * BF_SPATIAL_TAP_STRIDE;
	return queue_frames_of_newest(count, t, count, image_plane_tag, first_frame_id, device_ms,
		[=](Device &d, const FrameRecord &newest, bool cplx, uint32_t frames) {
			uint64_t run, field;
			bytes_of(newest, cplx, frames, run, field);
			if ((uint64_t)newest.points[0] * newest.points[1] * newest.points[2] > 0x7FFFFFFFull) return false;   /* the launches count a slice's voxels in 32 bits */
			const uint64_t need = (passes > 1u ? run : 0u) + d_fields * field;
			return need == 0 || d.ops.spatial_scratch.ensure(need);
		},
		[=](const QueuedRun &r) {
			FrameRecord shape; uint64_t run, field;
			for (int k = 0; k < 3; k++) shape.points[k] = r.points[k];
			bytes_of(shape, r.cplx, r.K, run, field);
			char *scratch = (char *)r.d->ops.spatial_scratch.ptr, *ring_out = (char *)r.ring + r.out_offset;
			float *d_field[2] = {(float *)(scratch + (passes > 1u ? run : 0u)), (float *)(scratch + (passes > 1u ? run : 0u) + field)};
			const uint32_t inner[3] = {1u, r.points[0], r.points[0] * r.points[1]}, outer[3] = {r.points[1] * r.points[2], r.points[2], 1u};
			const void *in = r.ring;
			for (uint32_t p = 0; p < passes; p++) {
				const uint32_t axis = axes[p];
				const bool to_ring = (passes - 1u - p) % 2u == 0;
				BfSpatialArgs a{};
				a.frames = r.K; a.cplx = r.cplx; a.stage = normalised ? (p == 0 ? 1u : 2u) : 0u; a.last = p + 1u == passes;
				a.inner = inner[axis]; a.extent = r.points[axis]; a.outer = outer[axis]; a.taps = n[axis];
				a.in_stride = r.out_stride; a.out_stride = r.out_stride; a.d_stride = field / r.K / sizeof(float);
				void *out = to_ring ? ring_out : scratch;
				const hipError_t e = bf_launch_spatial(in, p == 0 ? r.offsets : nullptr, out, p ? d_field[(p - 1u) % 2u] : nullptr,
				                                       normalised && !a.last ? d_field[p % 2u] : nullptr,
				                                       r.table + axis * BF_SPATIAL_TAP_STRIDE + BF_SPATIAL_TAP_FRONT, &a, r.s);
				if (e != hipSuccess) return e;
				in = out;
			}
			return hipSuccess;
		});
}

/* beamformer_hip_warp_last_frames: the `count` newest frames resampled at v + d(v), queued as `count` frames of their own (warp.hip).
 * One launch; the rotations and the field travel as the call's flat table (bf_warp_table_floats: within the table of a mix by the
 * limits lib_api.cpp has checked), the lattice's constants as kernel arguments.  No memory of its own. */
bool warp_last_frames(uint32_t count, const float *field, const uint32_t nodes[3], const float node_first[3], const float node_step[3],
                      const float *rotations, uint32_t interpolation, uint32_t edge, uint32_t image_plane_tag,
                      uint32_t *first_frame_id, float *device_ms)
{
	static_assert(BF_WARP_MAX_NODES == BEAMFORMER_HIP_MAX_WARP_NODES && BF_WARP_MAX_ENTRIES == BEAMFORMER_HIP_MAX_WARP_ENTRIES, "one limit");
	static_assert(sizeof(float) * (2u * BF_ENSEMBLE_MAX_FRAMES + 3u * BF_WARP_MAX_ENTRIES) <= sizeof(float) * 2 * BF_ENSEMBLE_MAX_FRAMES * BF_ENSEMBLE_MAX_FRAMES,
	              "the table of a warp fits the table of a mix");
	const uint32_t node_product = nodes[0] * nodes[1] * nodes[2];
	std::vector<float> table(bf_warp_table_floats(count, node_product));
	for (uint32_t n = 0; n < count; n++) {
		table[2u * n] = rotations ? rotations[2u * n] : 1.0f;
		table[2u * n + 1u] = rotations ? rotations[2u * n + 1u] : 0.0f;
	}
	std::memcpy(table.data() + 2u * count, field, sizeof(float) * 3u * count * node_product);
	BfWarpArgs a{};
	a.cubic = interpolation == BeamformerHipWarpInterpolation_Cubic; a.clamp = edge == BeamformerHipWarpEdge_Clamp;
	a.rotate = rotations != nullptr;
	a.direct = (ctx().das_path_mode & BeamformerHipDasPath_WarpDirect) != 0;
	for (int k = 0; k < 3; k++) {
		a.nodes[k] = nodes[k];
		if (nodes[k] > 1u) { a.node_first[k] = node_first[k]; a.inv_step[k] = 1.0f / node_step[k]; }
	}
	RunTable t; t.flat = table.data(); t.flat_floats = (uint32_t)table.size();
	return queue_frames_of_newest(count, t, count, image_plane_tag, first_frame_id, device_ms,
		[=](Device &, const FrameRecord &newest, bool cplx, uint32_t) {
			if ((uint64_t)newest.points[0] * newest.points[1] * newest.points[2] > 0x7FFFFFFFull) return false;   /* the kernel indexes a frame's voxels in 32 bits */
			for (uint32_t n = 0; n < count && rotations && !cplx; n++)
				if (rotations[2u * n + 1u] != 0.0f) return false;
			return true;
		},
		[=](const QueuedRun &r) {
			BfWarpArgs args = a;
			args.frames = r.K; args.cplx = r.cplx;
			for (int k = 0; k < 3; k++) args.points[k] = r.points[k];
			args.out_offset = r.out_offset; args.out_stride = r.out_stride;
			return bf_launch_warp(r.ring, r.offsets, r.table, &args, r.s);
		});
}

/* What beamformer_hip_queue_localisation_map and beamformer_hip_queue_track_map share: something made of a map that has been deposited
 * into, queued as ONE Float32 frame of the map's grid -- a run of one frame that has no source in the ring: the map is the library's own
 * buffer, so no placement can lie on what the launch reads.  The record carries the block of the newest frame of the last call that
 * deposited.  convert(run, out): the one launch. */
template <class Convert>
static bool queue_deposit_map(const FrameOps::DepositMap &map, uint32_t image_plane_tag, uint32_t *frame_id, float *device_ms, Convert convert)
{
	Context &c = ctx();
	if (!c.device_ready || c.device_count != 1 || !map.exists() || map.calls == 0) return set_error(BeamformerLibErrorKind_InvalidAccess);
	FrameRecord shape;
	for (int k = 0; k < 3; k++) shape.points[k] = map.points[k];
	shape.block = map.block;
	RunTable t; t.shape = &shape;
	return queue_frames_of_newest(0, t, 1, image_plane_tag, frame_id, device_ms, nothing_to_prepare,
		[=](const QueuedRun &r) { return convert(r, (float *)((char *)r.ring + r.out_offset)); });
}

/* beamformer_hip_queue_localisation_map: the map's counts times `scale` (frame_peaks.hip: the conversion) */
bool queue_localisation_map(float scale, uint32_t image_plane_tag, uint32_t *frame_id, float *device_ms)
{
	const FrameOps::DepositMap &map = ctx().devices[0].ops.map;
	const uint32_t *counts = (const uint32_t *)map.buffer.ptr;
	return queue_deposit_map(map, image_plane_tag, frame_id, device_ms, [=](const QueuedRun &r, float *out) {
		return bf_launch_localisation_convert(counts, out, r.elements, scale, r.s);
	});
}

/* beamformer_hip_queue_track_map: one component of the track map -- a mean displacement, the count, the squared mean speed
 * (frame_tracks.hip: the conversion) */
bool queue_track_map(uint32_t component, float scale, uint32_t min_pairs, uint32_t image_plane_tag, uint32_t *frame_id, float *device_ms)
{
	const FrameOps::DepositMap &map = ctx().devices[0].ops.tracks;
	const uint32_t *counts = (const uint32_t *)map.buffer.ptr;
	const void *sums = (const char *)map.buffer.ptr + map.sums_at();
	return queue_deposit_map(map, image_plane_tag, frame_id, device_ms, [=](const QueuedRun &r, float *out) {
		return bf_launch_track_convert(counts, sums, out, r.elements, component, min_pairs, scale, r.s);
	});
}

} // namespace bf
