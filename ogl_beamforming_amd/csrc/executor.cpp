/* executor.cpp -- device side of the in-process beamformer: RF ingest, per-frame stage
 * launches, frame ring, export, timings.
 *
 * Replaces the reference's two worker loops and their Vulkan plumbing:
 *   beamformer_rf_upload        (beamformer_core.c:1756-1805)  -> push_rf_and_compute: pinned
 *                                                                slot + H2D on a copy stream
 *                                                                + the ingest kernel
 *   complete_queue / Compute    (beamformer_core.c:1519-1677)  -> run_frame: stage launches in
 *                                                                stream order, one pass over
 *                                                                all channels
 *   complete_queue / Export     (beamformer_core.c:1468-1509)  -> export_last_frames
 *   beamformer_frame_next       (beamformer_core.c:440-466)    -> next_frames
 *   gpu_command_timestamp + coalesce_timing_table
 *                               (beamformer_core.c:1611-1655, :1683-1747) -> HIP event pairs
 * There is no CPU fallback: without a HIP device every entry point fails with
 * BeamformerLibErrorKind_SharedMemory.
 */
#include "context.h"
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <thread>

namespace bf {

static Context g_context;
Context &ctx() { return g_context; }

bool set_error(BeamformerLibErrorKind kind)
{
	g_context.last_error = kind;
	return false;
}

bool DeviceBuffer::ensure(size_t bytes)
{
	if (bytes <= size && ptr) return true;
	if (ptr) { (void)hipFree(ptr); ptr = nullptr; size = 0; }
	if (bytes == 0) bytes = 64;
	if (!HIP_OK(hipMalloc(&ptr, bytes))) { ptr = nullptr; return false; }
	size = bytes;
	return true;
}

void DeviceBuffer::release()
{
	if (ptr) (void)hipFree(ptr);
	ptr = nullptr; size = 0;
}

/* beamformer.c:196-228 picks the first of {4, 2, 1.5, 1} GiB that fits half the device heap;
 * on a 288 GB MI355X that is always 4 GiB, so the default needs no device query.
 * BEAMFORMER_HIP_FRAME_RING_BYTES overrides it (before first use). */
uint64_t default_frame_ring_bytes()
{
	if (const char *e = std::getenv("BEAMFORMER_HIP_FRAME_RING_BYTES")) {
		unsigned long long v = std::strtoull(e, nullptr, 0);
		if (v >= (1ull << 20)) return round_up(v, 64);
	}
	return 4ull << 30;
}

static bool init_one_device(Context &c, Device &d, int ordinal, uint32_t index)
{
	if (!HIP_OK(hipSetDevice(ordinal))) return false;
	if (!HIP_OK(hipStreamCreateWithFlags(&d.own_stream, hipStreamNonBlocking))) return false;
	if (!d.stream) d.stream = d.own_stream;
	if (!HIP_OK(hipStreamCreateWithFlags(&d.copy_stream, hipStreamNonBlocking))) return false;
	if (!HIP_OK(hipStreamCreateWithFlags(&d.peer_stream, hipStreamNonBlocking))) return false;
	for (uint32_t k = 0; k < BeamformerMaxRawDataFramesInFlight; k++) {
		if (!HIP_OK(hipEventCreateWithFlags(&d.rf_landed[k], hipEventDisableTiming))) return false;
		if (!HIP_OK(hipEventCreateWithFlags(&d.rf_consumed[k], hipEventDisableTiming))) return false;
		if (index != 0 && (!HIP_OK(hipEventCreate(&d.peer_copy_begin[k])) || !HIP_OK(hipEventCreate(&d.peer_copy_end[k])))) return false;
		d.consumed_pending[k] = false;
	}
	if (!d.ring.ensure(c.frame_ring_bytes)) return false;
	d.frames.assign(BeamformerMaxBacklogFrames, FrameRecord{});
	d.device = ordinal; d.index = index;
	return true;
}

/* Makes `dev` the device the executor functions act on. */
static bool select_device(uint32_t dev)
{
	Context &c = g_context;
	c.cur = &c.devices[dev];
	return HIP_OK(hipSetDevice(c.cur->device));
}

bool ensure_device()
{
	Context &c = g_context;
	if (c.device_ready) {
		c.cur = &c.devices[0];
		if (!HIP_OK(hipSetDevice(c.cur->device))) return set_error(BeamformerLibErrorKind_SharedMemory);
		return true;
	}
	int count = 0;
	if (!HIP_OK(hipGetDeviceCount(&count)) || count <= 0) return set_error(BeamformerLibErrorKind_SharedMemory);
	int      ordinals[kMaxDevices];
	uint32_t n = c.requested_count;
	if (n == 0) {
		const char *e = std::getenv("BEAMFORMER_HIP_DEVICE");
		if (!e) e = std::getenv("LOCAL_RANK");
		ordinals[0] = e ? std::atoi(e) : 0;
		n = 1;
	} else {
		for (uint32_t i = 0; i < n; i++) ordinals[i] = c.requested_devices[i];
	}
	for (uint32_t i = 0; i < n; i++)
		if (ordinals[i] < 0 || ordinals[i] >= count) return set_error(BeamformerLibErrorKind_SharedMemory);
	if (!c.frame_ring_bytes) c.frame_ring_bytes = default_frame_ring_bytes();
	bool ok = true;
	for (uint32_t i = 0; i < n && ok; i++) ok = init_one_device(c, c.devices[i], ordinals[i], i);
	/* peers copy the RF from the ingest device: ask whether each can reach it directly (xGMI) and enable that; a refusal is not an
	 * error -- hipMemcpyPeerAsync then stages the copy through host memory -- but it is remembered and reported
	 * (beamformer_hip_get_device_info), because a scaling run that silently went through the host explains nothing */
	for (uint32_t i = 0; i < n && ok; i++) c.devices[i].peer_access = 2;
	for (uint32_t i = 1; i < n && ok; i++) {
		if (c.devices[i].device == c.devices[0].device) continue;
		int can = 0;
		bool direct = HIP_OK(hipDeviceCanAccessPeer(&can, c.devices[i].device, c.devices[0].device)) && can;
		if (direct) {
			(void)hipSetDevice(c.devices[i].device);
			hipError_t e = hipDeviceEnablePeerAccess(c.devices[0].device, 0);
			direct = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
			/* and the other way (the ingest device's stream waits on the peer's events; some runtimes want both directions mapped) */
			(void)hipSetDevice(c.devices[0].device);
			hipError_t back = hipDeviceEnablePeerAccess(c.devices[i].device, 0);
			direct = direct && (back == hipSuccess || back == hipErrorPeerAccessAlreadyEnabled);
		}
		(void)hipGetLastError();
		c.devices[i].peer_access = direct ? 1 : 0;
		if (!direct) std::fprintf(stderr, "[beamformer] device %d has no peer access to device %d: RF copies to it are staged through host memory\n",
		                          c.devices[i].device, c.devices[0].device);
	}
	c.device_count = n;
	c.cur = &c.devices[0];
	c.device_ready = true;                      /* so that shutdown_device releases a partial set-up */
	if (!ok || !HIP_OK(hipSetDevice(c.devices[0].device))) { shutdown_device(); return set_error(BeamformerLibErrorKind_SharedMemory); }
	return true;
}

static void release_one_device(Device &d)
{
	if (d.device < 0) return;
	(void)hipSetDevice(d.device);
	(void)hipDeviceSynchronize();
	for (auto &p : d.plans) {
		p.hadamard_t.release(); p.hadamard_base.release(); p.readi_hadamard.release(); p.transmits.release();
		p.sparse.release(); p.mapping.release();
		for (auto &t : p.taps) t.release();
		p.taps.clear(); p.valid = false;
	}
	for (auto &b : d.raw_staging) b.release();
	for (auto &u : d.upload) {
		if (u.pinned) (void)hipHostFree(u.pinned);
		if (u.copied) (void)hipEventDestroy(u.copied);
		if (u.consumed) (void)hipEventDestroy(u.consumed);
		u = UploadSlot{};
	}
	if (d.copy_stream) (void)hipStreamDestroy(d.copy_stream);
	if (d.peer_stream) (void)hipStreamDestroy(d.peer_stream);
	d.copy_stream = d.peer_stream = nullptr;
	for (uint32_t k = 0; k < BeamformerMaxRawDataFramesInFlight; k++) {
		if (d.rf_landed[k])   (void)hipEventDestroy(d.rf_landed[k]);
		if (d.rf_consumed[k]) (void)hipEventDestroy(d.rf_consumed[k]);
		if (d.peer_copy_begin[k]) (void)hipEventDestroy(d.peer_copy_begin[k]);
		if (d.peer_copy_end[k])   (void)hipEventDestroy(d.peer_copy_end[k]);
		d.rf_landed[k] = d.rf_consumed[k] = d.peer_copy_begin[k] = d.peer_copy_end[k] = nullptr; d.consumed_pending[k] = false;
	}
	for (auto &b : d.rf) b.release();
	for (auto &b : d.scratch) b.release();
	d.ring.release(); d.pair_counter.release(); d.minmax_scratch.release(); d.sum_scratch.release();
	d.hercules_table.release(); d.hercules_pairs.release(); for (auto &b : d.burst_stage) b.release(); d.multi = PushRecord{};
	for (auto &vp : d.variant_plans) vp.clear();
	for (auto &ip : d.image_plans) { ip.ps.transmits.release(); ip.ps.sparse.release(); ip.ps.valid = false; ip.ps.das_parts.clear(); }
	d.readi_decoded.release(); d.das_decoded_bytes = 0;
	d.ops.release();
	d.views_table.release();
	if (d.views_pinned) (void)hipHostFree(d.views_pinned);
	if (d.views_copied) (void)hipEventDestroy(d.views_copied);
	d.views_pinned = nullptr; d.views_copied = nullptr; d.views_copy_pending = false;
	d.staged_tables.release(); d.staged_violations.release();
	for (auto &g : d.frame_exec) { if (g) (void)hipGraphExecDestroy(g); g = nullptr; }
	for (auto &g : d.graph_generation) g = 0;
	for (auto &t : d.timing) {
		if (t.created) for (auto &e : t.events) if (e) (void)hipEventDestroy(e);
		t = TimingSlot{};
	}
	if (d.own_stream) (void)hipStreamDestroy(d.own_stream);
	if (d.stream == d.own_stream || d.index != 0) d.stream = nullptr;   /* a caller's stream on the first device stays selected */
	d.own_stream = nullptr;
	d.frames.clear();
	d.ring_next_offset = 0; d.frame_counter = 0; d.rf_index = 0;
	d.have_sample = false; d.last_sampled_frame = 0; d.last_sampled_block = 0; d.replan_frame = 0;
	d.last_rf = nullptr; d.last_rf_bytes = 0; d.last_rf_slot = 0; d.peer_access = 2;
	d.das_input = nullptr; d.das_input_bytes = d.das_input_stride = 0; d.das_input_frames = 0;
	d.device = -1;
}

void shutdown_device()
{
	Context &c = g_context;
	if (!c.device_ready) return;
	for (uint32_t i = 0; i < kMaxDevices; i++) release_one_device(c.devices[i]);
	c.device_ready = false; c.device_count = 1; c.cur = &c.devices[0];
	c.push_sequence = 0;
	for (auto &b : c.blocks) b.dirty |= Dirty_Parameters;   /* plans are rebuilt on next use */
}

static bool upload(DeviceBuffer &dst, const void *src, size_t bytes, hipStream_t s)
{
	if (!dst.ensure(bytes ? bytes : 64)) return false;
	if (!bytes) return true;
	return HIP_OK(hipMemcpyAsync(dst.ptr, src, bytes, hipMemcpyHostToDevice, s));
}

static uint16_t half_bits_pm1(float v) { return v < 0 ? 0xBC00 : 0x3C00; }   /* +-1 as binary16 */

/* beamformer_commit_parameter_block (beamformer_core.c:1191-1287): replan when the block
 * changed and refresh the device-side tables. */
static PlanState *commit_block(uint32_t block)
{
	Context &c = g_context;
	Device  &d = *c.cur;
	ParameterBlock &pb = c.blocks[block];
	PlanState &ps = d.plans[block];
	if (ps.valid && !pb.dirty) return &ps;
	/* with several devices every one of them replans: the change reaches them through push_rf_and_compute,
	 * which commits the ingest device LAST -- only that commit clears the dirty bits */
	const bool clears_dirty = c.device_count == 1 || d.index == 0;

	std::string error;
	Plan plan;
	if (!build_plan(pb, plan, error, c.hilbert_enabled)) { ps.valid = false; ps.error = error; return nullptr; }
	ps.plan = std::move(plan);
	const BeamformerParameters &bp = pb.parameters;
	hipStream_t s = d.stream;

	/* a table a kernel of an earlier frame may still be reading must not be overwritten
	 * under it: replanning is rare, so simply drain the stream first */
	(void)hipStreamSynchronize(s);

	bool ok = true;
	ok &= upload(ps.mapping, pb.channel_mapping, sizeof(pb.channel_mapping), s);
	ok &= upload(ps.sparse,  pb.sparse_elements, sizeof(pb.sparse_elements), s);

	/* per-transmit constants (das.glsl:172-202) */
	uint32_t A = bp.acquisition_count;
	ps.transmit_table = build_transmit_table(pb);
	ok &= upload(ps.transmits, ps.transmit_table.data(), sizeof(BfTransmit) * A, s);

	if (!ps.plan.hadamard_t.empty())
		ok &= upload(ps.hadamard_t, ps.plan.hadamard_t.data(), sizeof(float) * ps.plan.hadamard_t.size(), s);
	if (!ps.plan.hadamard_base.empty())
		ok &= upload(ps.hadamard_base, ps.plan.hadamard_base.data(), sizeof(float) * ps.plan.hadamard_base.size(), s);
	ps.readi_bits.clear();
	for (float v : ps.plan.readi_hadamard) ps.readi_bits.push_back(half_bits_pm1(v));
	if (!ps.readi_bits.empty())
		ok &= upload(ps.readi_hadamard, ps.readi_bits.data(), sizeof(uint16_t) * ps.readi_bits.size(), s);

	for (auto &t : ps.taps) t.release();
	ps.tap_tables.clear();
	ps.taps.assign(ps.plan.stages.size(), DeviceBuffer{});
	for (size_t i = 0; i < ps.plan.stages.size(); i++) {
		const Stage &st = ps.plan.stages[i];
		if (st.kind == BeamformerShaderKind_Filter || st.kind == BeamformerShaderKind_Demodulate ||
		    st.kind == BeamformerShaderKind_Hilbert) {
			/* taps, then -- for Demodulate -- the window-local phasors {cos, -sin}(2 pi fd index / (fs/2))
			 * of filter.glsl:99-107, in the kernel's own f32 expression */
			ps.tap_tables.emplace_back(st.filter.taps);
			std::vector<float> &table = ps.tap_tables.back();
			if (st.kind == BeamformerShaderKind_Demodulate) {
				const uint32_t window = ps.plan.decimation * 64 + (uint32_t)st.filter.length - 1;
				const float fd = bp.demodulation_frequency, fs = bp.sampling_frequency / 2;
				for (uint32_t index = 0; index < window; index++) {
					float arg = 6.28318530717958647692f * fd * (float)index / fs;
					table.push_back(cosf(arg));
					table.push_back(-sinf(arg));
				}
			}
			ok &= upload(ps.taps[i], table.data(), sizeof(float) * table.size(), s);
		}
	}
	if (ps.plan.intermediate_bytes) {
		ok &= d.scratch[0].ensure(ps.plan.intermediate_bytes + 64);
		ok &= d.scratch[1].ensure(ps.plan.intermediate_bytes + 64);
	}
	/* host vectors above must outlive the async copies out of pageable memory */
	ok &= HIP_OK(hipStreamSynchronize(s));
	if (!ok) { ps.valid = false; ps.error = "device allocation or upload failed"; return nullptr; }
	if (clears_dirty) pb.dirty = 0;
	ps.valid = true;
	ps.generation++;
	ps.das_parts.clear();
	d.variant_plans[block].clear();            /* a variants push's derived decisions were made for the plan that has just gone */
	return &ps;
}

/* The derived block of a READI image push (das_select.h: derive_readi_image) beside the block's own plan state `ps`: its plan, the
 * transmit table of its G x A transmits on the device, and -- filled by frame_das_parts -- its own DAS decision.  Rebuilt when the block
 * has been replanned since (a dirtied block drops it with its plan). */
static ImagePlanState *commit_image_plan(uint32_t block, PlanState *ps)
{
	Context &c = g_context;
	Device  &d = *c.cur;
	ImagePlanState &ip = d.image_plans[block];
	if (ip.ps.valid && ip.source_generation == ps->generation) return &ip;
	hipStream_t s = d.stream;
	(void)hipStreamSynchronize(s);          /* as commit_block: an earlier frame may still read the tables */
	derive_readi_image(c.blocks[block], ps->plan, ip.pb, ip.ps.plan);
	ip.ps.transmit_table = build_transmit_table(ip.pb);
	bool ok = upload(ip.ps.transmits, ip.ps.transmit_table.data(), sizeof(BfTransmit) * ip.ps.transmit_table.size(), s);
	ok &= upload(ip.ps.sparse, ip.pb.sparse_elements, sizeof(ip.pb.sparse_elements), s);
	ok &= HIP_OK(hipStreamSynchronize(s));
	ip.ps.das_parts.clear();
	ip.ps.generation = ip.source_generation = ps->generation;
	ip.ps.valid = ok;
	return ok ? &ip : nullptr;
}

/* One frame a push queues.  The push describes it -- which RF frame's DAS input it reads, its grid, the parts that compute it
 * (das_select.h) and whether the push's fused launch covers it --; walk_plan places it in the ring, resolves `in` and `out` and runs it. */
struct DasJob {
	uint32_t        rf_frame;       /* reads the DAS input of this RF frame of the push */
	const uint32_t *points;         /* its grid, and the tag its record carries */
	uint32_t        tag;
	uint32_t        z_first;
	const std::vector<DasDecision> *parts;   /* null: no DAS runs for the frame (no DAS stage, an empty slab) and it stays zero */
	bool            fused;          /* the push's fused launch covers it; else it gets its own launch(es), the kernels of a single push */
	int32_t         group;          /* >= 0: its launches run with this BfDasArgs::readi_group; -1: the block's */
	/* the walk's: */
	const char     *in;
	char           *out;
	uint32_t        path;           /* the kernel that ran its main part */
};

/* What the ring's placement rule needs of a frame: its grid and the tag its record carries.  A push's frames are DasJobs; the frames
 * mix_last_frames writes are no jobs.  shape_of(k): frame k of the run. */
struct FrameShape { const uint32_t *points; uint32_t tag; };

/* The bytes of a run of frames, contiguous in the frame ring, each rounded to 64 bytes (frame_run_bytes per frame: saturating).  False:
 * the run does not fit `ring` bytes. */
template <class ShapeOf>
static bool run_bytes_of(ShapeOf shape_of, uint32_t count, uint64_t voxel_bytes, uint64_t ring, uint64_t &total)
{
	total = 0;
	for (uint32_t k = 0; k < count; k++) {
		uint64_t frame;
		if (!frame_run_bytes(shape_of(k).points, nullptr, 1, voxel_bytes, ring, frame) || frame > ring - total) return false;
		total += frame;
	}
	return true;
}

static bool job_run_bytes(const DasJob *jobs, uint32_t count, uint64_t voxel_bytes, uint64_t ring, uint64_t &total)
{
	return run_bytes_of([jobs](uint32_t k) { return FrameShape{jobs[k].points, jobs[k].tag}; }, count, voxel_bytes, ring, total);
}

/* beamformer_frame_next (beamformer_core.c:440-466), for a run of `count` frames, contiguous in the ring, each rounded to 64 bytes: frame
 * k has shape_of(k)'s points and tag.  A run that would straddle the end starts again at offset 0; the records it overwrites stop being
 * exportable.  Consecutive ids, each frame's timing slot named in its record.  Returns the first, or null when the run does not fit the
 * ring; total: the bytes of the whole run. */
template <class ShapeOf>
static FrameRecord *place_frames(ShapeOf shape_of, uint32_t count, bool complex_frame, uint32_t block, uint64_t &total)
{
	Device &d = *g_context.cur;
	const int kind = complex_frame ? BeamformerDataKind_Float32Complex : BeamformerDataKind_Float32;
	if (count == 0 || !run_bytes_of(shape_of, count, (uint64_t)bf_kind_byte_size[kind], d.ring.size, total)) return nullptr;
	if (d.ring_next_offset > d.ring.size - total) d.ring_next_offset = 0;
	/* records whose storage the run reuses stop being exportable: one pass for the run's whole byte range (the run's own records are
	 * written below, after it) */
	for (FrameRecord &old : d.frames)
		if (old.bytes && old.offset < d.ring_next_offset + total && d.ring_next_offset < old.offset + old.bytes) old.bytes = 0;
	FrameRecord *first = nullptr;
	for (uint32_t k = 0; k < count; k++) {
		const FrameShape shape = shape_of(k);
		const uint32_t *n = shape.points;
		const uint64_t bytes = round_up((uint64_t)n[0] * n[1] * n[2] * (uint64_t)bf_kind_byte_size[kind], 64);
		uint64_t id = d.frame_counter++;
		FrameRecord *f = &d.frames[id % d.frames.size()];
		f->offset = d.ring_next_offset; f->bytes = bytes;
		f->points[0] = n[0]; f->points[1] = n[1]; f->points[2] = n[2];
		f->data_kind = kind; f->id = (uint32_t)id; f->block = block; f->failed = false;
		f->tag = shape.tag;
		f->timing_slot = (int)(id % kTimingSlots);
		d.ring_next_offset += bytes;
		if (k == 0) first = f;
	}
	return first;
}

/* the frames of a push: job k's points and tag */
static FrameRecord *next_frames(const DasJob *jobs, uint32_t count, bool complex_frame, uint32_t block, uint64_t &total)
{
	return place_frames([jobs](uint32_t k) { return FrameShape{jobs[k].points, jobs[k].tag}; }, count, complex_frame, block, total);
}

/* A timed HIP event costs ~4 us of stream time on this runtime (measured: a 0.26 MB / 256 x 256
 * frame takes 36.5 us with its five records and 15.7 us without), nothing next to a 3-D volume
 * and more than the kernels of a real-time 2-D frame.  Small frames therefore record their
 * per-stage events on one frame in kTimingSamplePeriod; the frames in between run with no event
 * at all and report the newest sampled timings in the stats table. */
constexpr uint64_t kTimingSamplePeriod = 8;
constexpr uint64_t kSmallFrameBytes    = 8ull << 20;
/* A copy-engine transfer and each cross-queue dependency cost 40-60 us of latency on this runtime (tools/h2d_probe.cpp: 0.26 MB pinned
 * H2D + a kernel = 114 us per frame), more than a small frame's compute, so host uploads (a single frame's, a whole burst's) under
 * kOverlapBytes skip the copy engine: the ingest kernel reads the pinned slot in place over PCIe, in order on the compute stream. */
constexpr uint64_t kOverlapBytes       = 8ull << 20;

static bool ensure_events(TimingSlot &t)
{
	if (t.created) return true;
	for (auto &e : t.events) if (!HIP_OK(hipEventCreate(&e))) return set_error(BeamformerLibErrorKind_SharedMemory);
	t.created = true;
	return true;
}

static bool record(TimingSlot &t, uint32_t index, hipStream_t s)
{
	if (!t.sampled) return true;
	return HIP_OK(hipEventRecord(t.events[index], s));
}

/* segment k of a slot's timings is bracketed by events[k] and events[k+1]: closes the one that ran since the last record as `kind` */
static void segment(TimingSlot &t, uint32_t kind, hipStream_t s)
{
	if (t.count < BEAMFORMER_HIP_MAX_TIMED_STAGES) {
		t.kinds[t.count++] = kind;
		record(t, t.count, s);
	}
}

static bool run_frame_stages(uint32_t block, const void *rf, int64_t rf_bytes, bool ingest_timed);

/* One pre-DAS stage: stage i of the plan reads `cur` (cur_elements_bytes: what may be read there, per frame) and writes `out`.  A burst
 * passes its frame count and the byte strides from frame to frame of input and output: one launch (the filters: one per chunk of frames
 * that fits the grid, stages.hip), each frame addressed and bounded as a single frame is. */
static bool launch_stage(PlanState *ps, const BeamformerParameters &bp, size_t i, const void *cur, int64_t cur_elements_bytes, void *out, hipStream_t s,
                         uint32_t frames = 1, uint64_t in_frame_bytes = 0, uint64_t out_frame_bytes = 0)
{
	Context &c = g_context;
	const Plan &plan = ps->plan;
	const Stage &st = plan.stages[i];
	const uint32_t C = plan.channels, A = plan.acquisitions, Sd = plan.das_samples;
	bool ok = true;
	switch (st.kind) {
	case BeamformerShaderKind_Reshape:{
		BfReshapeArgs a{};
		a.size[0] = Sd; a.size[1] = C; a.size[2] = A;                          /* beamformer_core.c:975-977 */
		for (int k = 0; k < 3; k++) { a.in_stride[k] = st.in_stride[k]; a.out_stride[k] = st.out_stride[k]; }
		a.in_kind = st.in_kind; a.out_kind = st.out_kind;
		a.interleave = !bf_kind_complex[st.in_kind] && bf_kind_complex[st.out_kind];
		a.in_elements = cur_elements_bytes / bf_kind_byte_size[st.in_kind];
		a.left  = cur;
		a.right = (const char *)cur + (size_t)Sd * C * A * (size_t)bf_kind_byte_size[st.in_kind];   /* :1384-1385 */
		a.out = out;
		a.frames = frames; a.in_frame_bytes = in_frame_bytes; a.out_frame_bytes = out_frame_bytes;
		ok = HIP_OK(bf_launch_reshape(&a, s));
	}break;
	case BeamformerShaderKind_Decode:{
		BfDecodeArgs a{};
		a.in = cur; a.out = out;
		a.hadamard_t = (const float *)ps->hadamard_t.ptr;
		a.hadamard_base_order = (c.das_path_mode & BeamformerHipDasPath_DenseDecode) ? 0 : plan.hadamard_base_order;
		a.hadamard_base = a.hadamard_base_order ? (const float *)ps->hadamard_base.ptr : nullptr;
		a.transmit_count = A; a.channel_count = C; a.sample_count = Sd;
		for (int k = 0; k < 3; k++) a.out_stride[k] = st.out_stride[k];
		a.in_kind = st.in_kind; a.out_kind = st.out_kind;
		a.frames = frames; a.in_frame_bytes = in_frame_bytes; a.out_frame_bytes = out_frame_bytes;
		ok = HIP_OK(bf_launch_decode(&a, s));
	}break;
	case BeamformerShaderKind_Hilbert:{
		BfFilterArgs a{};
		a.in = cur; a.out = out;
		a.coefficients  = (const float *)ps->taps[i].ptr;
		a.filter_length = (uint32_t)st.filter.length;
		a.sample_count  = Sd;
		for (int k = 0; k < 3; k++) { a.in_stride[k] = st.in_stride[k]; a.out_stride[k] = st.out_stride[k]; }
		a.in_elements = cur_elements_bytes / bf_kind_byte_size[st.in_kind];
		a.channels = C; a.transmits = A;
		a.in_kind = st.in_kind; a.out_kind = st.out_kind;
		a.frames = frames; a.in_frame_bytes = in_frame_bytes; a.out_frame_bytes = out_frame_bytes;
		ok = HIP_OK(bf_launch_hilbert(&a, s));
	}break;
	case BeamformerShaderKind_Filter:
	case BeamformerShaderKind_Demodulate:{
		bool demod = st.kind == BeamformerShaderKind_Demodulate;
		BfFilterArgs a{};
		a.in = cur; a.out = out;
		a.coefficients   = (const float *)ps->taps[i].ptr;
		a.phasors        = demod ? a.coefficients + st.filter.taps.size() : nullptr;
		a.filter_length  = (uint32_t)st.filter.length;
		a.complex_filter = st.filter.complex_taps;
		a.demodulate     = demod;
		a.decimation     = demod ? plan.decimation : 1;                          /* :846 */
		a.sample_count   = Sd;                                                  /* :845 */
		bool deinterleave = bf_kind_complex[st.in_kind] && !bf_kind_complex[st.out_kind];
		a.batch_sample_count = deinterleave ? C * Sd * A : 0;                   /* :848-851 */
		if (demod) {                                                            /* :870-873 */
			a.demodulation_frequency = bp.demodulation_frequency;
			a.sampling_frequency     = bp.sampling_frequency / 2;
		}
		for (int k = 0; k < 3; k++) { a.in_stride[k] = st.in_stride[k]; a.out_stride[k] = st.out_stride[k]; }
		a.in_elements = cur_elements_bytes / bf_kind_byte_size[st.in_kind];
		a.channels = C; a.transmits = A;
		a.in_kind = st.in_kind; a.out_kind = st.out_kind;
		a.frames = frames; a.in_frame_bytes = in_frame_bytes; a.out_frame_bytes = out_frame_bytes;
		ok = HIP_OK(bf_launch_filter(&a, s));
	}break;
	default: break;
	}
	return ok;
}


/* The DAS decision(s) of a plan's frames over planes [zfirst, zfirst + zcount): computed once per plan / shard / path mode / hook change
 * (das_select.cpp) and reused by every frame after it.  Null: no DAS runs -- the plan has no DAS stage, or there are no planes. */
static const std::vector<DasDecision> *frame_das_parts(PlanState *ps, const ParameterBlock &pb, uint32_t zfirst, uint32_t zcount)
{
	Context &c = g_context;
	if (ps->plan.das_index < 0 || !zcount) return nullptr;
	std::vector<DasDecision> &parts = ps->das_parts;
	if (parts.empty() || !parts[0].valid || parts[0].generation != ps->generation || ps->das_z_first != zfirst || ps->das_z_count != zcount ||
	    parts[0].mode_asked != c.das_path_mode || parts[0].hooks_version != hooks().version) {
		decide_das_parts(pb, ps->plan, ps->transmit_table, zfirst, zcount, c.das_path_mode, parts);
		for (DasDecision &dd : parts) { dd.generation = ps->generation; dd.mode_asked = c.das_path_mode; }
		ps->das_z_first = zfirst; ps->das_z_count = zcount;
	}
	return &parts;
}

/* the plan's device tables, which every DAS launch reads */
static void bind_tables(const PlanState *ps, BfDasArgs &a)
{
	a.transmits       = (const BfTransmit *)ps->transmits.ptr;
	a.sparse_elements = (const int16_t *)ps->sparse.ptr;
	a.readi_hadamard  = (const uint16_t *)ps->readi_hadamard.ptr;
}

/* One part of one frame's DAS stage (das_select.h: a frame is one part unless the row-end rule cut it): the kernel `dd` names on the DAS
 * input `cur`, writing the part's planes at `out`.  part_path: the kernel that ran where a missing buffer sent the part to another one. */
static bool launch_das_part(PlanState *ps, const DasDecision &dd, const void *cur, void *out, uint64_t out_bytes, uint32_t *frame_counters,
                            hipStream_t s, uint32_t &part_path, int32_t readi_group = -1)
{
	Device &d = *g_context.cur;
	bool ok = true;
	BfDasArgs a = dd.a;
	a.rf  = cur;
	a.out = out;
	bind_tables(ps, a);
	if (readi_group >= 0) a.readi_group = (uint32_t)readi_group;       /* a READI sweep's frame: its only difference from a single push */

	if (dd.path == DasPath_Zero) {
		ok &= HIP_OK(hipMemsetAsync(a.out, 0, out_bytes, s));
	} else {
		/* 64 zero bytes right behind the DAS input (every buffer it can live in is allocated with that much slack): the
		 * gather target of out-of-range lanes */
		const uint64_t used = dd.das_input_bytes;
		if (dd.path != DasPath_General) ok &= HIP_OK(hipMemsetAsync((char *)const_cast<void *>(cur) + used, 0, 64, s));
		switch (dd.path) {
		case DasPath_Staged:
		case DasPath_Gather:{
			BfSeparableArgs sep = dd.sep;
			bool staged = dd.path == DasPath_Staged;
			if (staged && sep.uniform) {
				/* the wave-uniform transmit tables live in global memory: one slice per (lateral tile row, plane), written per frame;
				 * no memory: the shape with the tables in LDS, else the gather kernel with its own geometry */
				const uint64_t table_bytes = (uint64_t)sep.table_stride * sep.tiles[1] * sep.tiles[2];
				if (d.staged_tables.ensure(table_bytes)) {
					sep.tables = d.staged_tables.ptr;
					ok &= HIP_OK(bf_launch_das_staged_tables(&a, &sep, s));
				} else if (dd.has_lds_tables) {
					sep = dd.sep_lds_tables;
				} else {
					sep = dd.sep_gather; staged = false;
				}
			}
			if (staged) {
				/* window positions outside the staged window are counted (range-checked loop only: STAGED_CHECKED) */
				sep.violations = frame_counters;
				ok &= HIP_OK(!ps->plan.iq_pipeline ? bf_launch_das_staged_real(&a, &sep, s) :
				             a.interpolation == 2 ? bf_launch_das_staged_cubic(&a, &sep, s) : bf_launch_das_staged(&a, &sep, s));
				part_path = DasPath_Staged;
			} else {
				ok &= HIP_OK(bf_launch_das_separable(&a, &sep, s));
				part_path = DasPath_Gather;
			}
		}break;
		case DasPath_Hercules:{
			BfHerculesArgs hq = dd.herc;
			if (d.hercules_table.ensure(((size_t)hq.table_pitch + 2) * a.size[1] * sizeof(float))) {
				hq.pairs = nullptr;
				const uint64_t prepared = used * (a.interpolation == 2 ? 4u : 2u);      /* cubic: four coefficients per sample, 32 bytes */
				if (dd.hercules_prepared && d.hercules_pairs.ensure(prepared + 64)) {
					hq.pairs = d.hercules_pairs.ptr;
					hq.zero_offset = (uint32_t)prepared;
				}
				hq.table    = (float *)d.hercules_table.ptr;
				hq.extremes = hq.table + (size_t)hq.table_pitch * a.size[1];
				ok &= HIP_OK(bf_launch_das_hercules(&a, &hq, s));
			} else {
				ok &= HIP_OK(bf_launch_das(&a, s));                                     /* no memory for the row table: the general kernel */
				part_path = DasPath_General;
			}
		}break;
		case DasPath_Factored:
			ok &= HIP_OK(bf_launch_das_factored(&a, s));
			break;
		case DasPath_Tile:
			/* (block, channel chunk) pairs served from staged windows, and those the kernel sent through its gather loop: words 1, 2 */
			a.tile_counters = frame_counters ? frame_counters + 1 : nullptr;
			ok &= HIP_OK(bf_launch_das_tile(&a, s));
			break;
		default:
			ok &= HIP_OK(bf_launch_das(&a, s));
			break;
		}
	}
	return ok;
}

/* One frame.  With frame graphs on (beamformer_hip_enable_frame_graphs; BASELINE.json configs[4]: "hipGraph-
 * captured frame"; the reference's analogue is the one command list it records per frame,
 * beamformer_core.c:1570-1620) the stage launches are captured into a hipGraph instead of being enqueued:
 * every frame is captured (the frame-ring slot and the RF slot move from frame to frame, so kernel arguments
 * change), the block's instantiated graph is updated in place from the capture (hipGraphExecUpdate: same
 * topology, new arguments; re-instantiated when the topology changed) and launched.  The first frame of a
 * plan runs uncaptured so that every allocation a stage needs exists before anything is captured.  Per-stage
 * events cannot be recorded inside a graph: a graph frame times as one segment, reported under DAS. */
static bool run_frame(uint32_t block, const void *rf, int64_t rf_bytes, bool ingest_timed)
{
	Context &c = g_context;
	Device  &d = *c.cur;
	if (!c.frame_graphs || c.device_count != 1 || c.count_pairs) return run_frame_stages(block, rf, rf_bytes, ingest_timed);
	PlanState *ps = commit_block(block);                   /* a replan drains the stream: never inside a capture */
	if (!ps) return set_error(BeamformerLibErrorKind_InvalidComputeStage);
	if (d.graph_generation[block] != ps->generation) {
		d.graph_generation[block] = ps->generation;
		if (d.frame_exec[block]) { (void)hipGraphExecDestroy(d.frame_exec[block]); d.frame_exec[block] = nullptr; }
		return run_frame_stages(block, rf, rf_bytes, ingest_timed);
	}
	hipStream_t s = d.stream;
	TimingSlot &t = d.timing[d.frame_counter % kTimingSlots];
	t.failed = false;
	if (!ensure_events(t)) return false;
	const bool sampled = t.sampled;
	const uint32_t first = ingest_timed ? 1u : 0u;          /* events[0] -> events[1] is the caller's ingest segment */
	if (sampled && !HIP_OK(hipEventRecord(t.events[first], s))) return set_error(BeamformerLibErrorKind_InvalidAccess);
	t.sampled = false;                                      /* no event records inside the capture */
	bool ok = HIP_OK(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
	if (!ok) { t.sampled = sampled; return set_error(BeamformerLibErrorKind_InvalidAccess); }
	ok = run_frame_stages(block, rf, rf_bytes, ingest_timed);
	hipGraph_t graph = nullptr;
	bool ended = HIP_OK(hipStreamEndCapture(s, &graph));
	t.sampled = sampled;
	if (!ok || !ended || !graph) { if (graph) (void)hipGraphDestroy(graph); return ok ? set_error(BeamformerLibErrorKind_InvalidAccess) : false; }
	if (d.frame_exec[block]) {
		hipGraphNode_t bad = nullptr; hipGraphExecUpdateResult why;
		if (!HIP_OK(hipGraphExecUpdate(d.frame_exec[block], graph, &bad, &why))) {
			(void)hipGetLastError();
			(void)hipGraphExecDestroy(d.frame_exec[block]); d.frame_exec[block] = nullptr;
		}
	}
	if (!d.frame_exec[block]) {
		ok = HIP_OK(hipGraphInstantiate(&d.frame_exec[block], graph, nullptr, nullptr, 0));
		c.graph_instantiations++;
	}
	(void)hipGraphDestroy(graph);
	ok = ok && HIP_OK(hipGraphLaunch(d.frame_exec[block], s));
	c.graph_frames += ok;
	/* the frame as one timed segment */
	t.count = 0;
	if (ingest_timed) t.kinds[t.count++] = kStageIngest;
	t.kinds[t.count++] = (uint32_t)BeamformerShaderKind_DAS;
	if (sampled) ok = ok && HIP_OK(hipEventRecord(t.events[t.count], s));
	return ok || set_error(BeamformerLibErrorKind_InvalidAccess);
}

/* All parts of one frame's DAS stage: the frame's DAS input at `cur`, its ring slot at `out`.  head_path: the kernel that ran the main part. */
static bool launch_frame_parts(PlanState *ps, const std::vector<DasDecision> &parts, uint32_t zfirst, uint64_t plane_bytes, const void *cur, char *out,
                               uint32_t *frame_counters, hipStream_t s, uint32_t &head_path, int32_t readi_group = -1)
{
	const DasDecision &head = main_part(parts);
	bool ok = true;
	for (const DasDecision &dd : parts) {
		uint32_t part_path = (uint32_t)dd.path;
		ok &= launch_das_part(ps, dd, cur, out + (uint64_t)(dd.z_first - zfirst) * plane_bytes, dd.z_count * plane_bytes, frame_counters, s, part_path, readi_group);
		if (&dd == &head && dd.path != DasPath_Zero) head_path = part_path;
	}
	return ok;
}

/* The DAS fields of a frame's row of the timing table; parts == null: no DAS kernel ran for the frame (no DAS stage, an empty slab). */
static void fill_das_fields(TimingSlot &t, uint64_t id, const std::vector<DasDecision> *parts, const uint32_t points[3], bool iq, uint32_t das_path,
                            uint64_t violations_slot)
{
	const uint32_t interpolation = parts ? main_part(*parts).a.interpolation : 0;
	t.frame_id = id;
	t.das_voxels = parts ? (uint64_t)points[0] * points[1] * points[2] : 0;
	t.das_taps = !parts ? 0 : interpolation == 0 ? 1 : interpolation == 1 ? 2 : 4;
	t.das_sample_bytes = !parts ? 0 : iq ? 8 : 4;
	t.das_path = parts ? das_path : 0;
	t.das_row_end_planes = parts ? row_end_planes(*parts) : 0;
	t.violations_slot = violations_slot;
}

/* The fused launch of a push: one kernel launch (or one per RF frame) that computes every job marked `fused`.  ONE tagged description;
 * walk_plan dispatches it through its one switch.  The pointers are the routes (das_select.h) of the kinds that name them. */
struct FusedLaunch {
	enum Kind {
		None,               /* every frame gets its own launch(es) */
		Burst,              /* das_burst.hip: every frame of a burst */
		ReadiSweep,         /* das_burst.hip, das_readi_burst_kernel: every frame of a READI sweep, frame k under groups[k] */
		Views,              /* das_views.hip: the views the route takes, from the one RF frame */
		Variants,           /* das_variants.hip: the variants the route takes, from the one RF frame */
		BurstViews,         /* das_burst_views.hip, once: the views the route takes, of every RF frame (a burst views push, rung 1) */
		ViewsPerRfFrame,    /* das_views.hip once per RF frame, on that frame's jobs and its slice of the input (a burst views push, rung 2) */
	} kind = None;
	const BurstDecision    *burst = nullptr;
	const ViewsDecision    *views = nullptr;
	const VariantsDecision *variants = nullptr;
	const uint32_t         *groups = nullptr;
};

/* A push, as walk_plan and push_frames run it; every member is assigned by name.
 * The RF frames and the buffers the pre-DAS stages run on: frame k of every buffer k * that buffer's stride further on (one frame:
 * stride 0).  The single push fills them in run_frame_stages, push_frames for every other push.
 * The frames: the jobs the push queues, in id order, the plan state their DAS launches bind, the fused launch that covers the jobs
 * marked `fused`, the decode step ahead of DAS.  The push_* function fills them, and what of its upload and record is its own. */
struct Push {
	uint32_t      rf_frames = 1;
	const void   *in = nullptr;         /* the first stage's input, and what it may read of a frame there */
	uint64_t      in_stride = 0;
	int64_t       in_bound = 0;
	DeviceBuffer *stage = nullptr;      /* the ping-pong pair the pre-DAS stages write */
	uint64_t      stage_stride = 0;     /* 0: a stage may read its predecessor's whole buffer; else its frame's stride */
	TimingSlot   *t = nullptr;          /* owns the events; its ingest segment (or events[0]) is already recorded */
	DasJob       *jobs = nullptr;
	uint32_t      frames = 1;
	PlanState    *das_ps = nullptr;     /* whose device tables the DAS launches bind: the block's own; a READI image's derived block's.  (A variant's
	                                       derived decision is its job's `parts`; the tables it binds do not depend on its values and are the
	                                       block's: context.h, VariantPlanState) */
	FusedLaunch   fused;
	const uint32_t *decode_groups = nullptr;   /* the decode step: the rf_frames DAS inputs are decoded across the acquisitions by these group ids
	                                              (readi_decode.hip) and the ONE job reads the result */
	bool          fails_on_flag = false;       /* path flag 0x2000 fails the DAS step once the ids are taken */
	PushRecord::Kind kind = PushRecord::None;
	uint32_t      rf_frame_size = 0;    /* rf_frames RF frames back to back, each this many bytes of the caller's */
	uint64_t      decoded_bytes = 0;    /* the decode step's output */
	float         decide_us = 0;
};

/* The small tables some launches read (a views push's rows and prefix table, a variants push's rows, the group ids of a READI sweep or
 * image) go to d.views_table through pinned memory on the push's stream, read in place by a small kernel (no copy engine:
 * bf_launch_views_table); push_frames grew both.  `fill` writes the `bytes` into the pinned memory once the copy that last read it has
 * passed. */
template <class Fill> static bool stage_table(size_t bytes, hipStream_t s, Fill fill)
{
	Device &d = *g_context.cur;
	if (d.views_copy_pending) { (void)hipEventSynchronize(d.views_copied); d.views_copy_pending = false; }
	fill(d.views_pinned);
	void *mapped = nullptr;
	bool ok = HIP_OK(hipHostGetDevicePointer(&mapped, d.views_pinned, 0));
	if (ok) ok &= HIP_OK(bf_launch_views_table(d.views_table.ptr, mapped, (uint32_t)bytes, s));
	d.views_copy_pending = HIP_OK(hipEventRecord(d.views_copied, s));
	return ok && d.views_copy_pending;
}

static bool stage_group_ids(const uint32_t *groups, uint32_t N, hipStream_t s)
{
	return stage_table(sizeof(uint32_t) * N, s, [&](void *pinned) { std::memcpy(pinned, groups, sizeof(uint32_t) * N); });
}

/* The burst kernel (das_burst.hip): N frames, frame k at k * the strides of input and output, in one launch.  `groups`: the READI sweep
 * kernel (das_readi_burst_kernel) instead -- the same launch with the frames' group ids staged ahead of it. */
static bool launch_burst_kernel(PlanState *ps, const BurstDecision &route, const DasJob &first, const uint32_t *groups, uint32_t N, uint64_t in_stride,
                                uint64_t out_stride, hipStream_t s)
{
	BfDasArgs a = route.a;
	a.rf = first.in; a.out = first.out;
	bind_tables(ps, a);
	BfReadiSweepArgs b{};
	b.burst.frame_count = N; b.burst.rf_stride = in_stride; b.burst.out_stride = out_stride;
	b.groups = (const uint32_t *)g_context.cur->views_table.ptr;
	if (!groups) return HIP_OK(bf_launch_das_burst(&a, &b.burst, s));
	return stage_group_ids(groups, N, s) && HIP_OK(bf_launch_das_readi_sweep(&a, &b, s));
}

/* The variants kernel (das_variants.hip): the variants the route has it take, from the ONE DAS input on the block's grid, in one launch --
 * their rows staged ahead of it.  Variant k's job is jobs[k]. */
static bool launch_variants_kernel(PlanState *ps, const VariantsDecision &route, const DasJob *jobs, uint32_t K, hipStream_t s)
{
	Device &d = *g_context.cur;
	const uint32_t n = route.kernel_variants;
	bool ok = stage_table(sizeof(BfVariantRow) * n, s, [&](void *pinned) {
		BfVariantRow *rows = (BfVariantRow *)pinned;
		for (uint32_t k = 0, r = 0; k < K; k++) {
			if (!route.taken[k]) continue;
			rows[r] = route.rows[r];
			rows[r].out_offset = (uint64_t)(jobs[k].out - jobs[0].out);
			r++;
		}
	});
	BfDasArgs a = route.a;
	a.rf = jobs[0].in; a.out = jobs[0].out;
	bind_tables(ps, a);
	if (ok) ok &= HIP_OK(bf_launch_das_variants(&a, (const BfVariantRow *)d.views_table.ptr, n, s));
	return ok;
}

/* The views kernel (das_views.hip): the views the route has it take, from the ONE DAS input, in one launch -- their rows and the prefix
 * table staged ahead of it.  View k's job is jobs[k * step] (a views push: step 1).  fused_frames: a burst views push's fused launch
 * (das_burst.hip: das_burst_views_kernel) instead -- that many RF frames, in_stride apart, view k's frames
 * jobs[k * step .. k * step + fused_frames - 1]. */
static bool launch_views_kernel(PlanState *ps, const ViewsDecision &route, const DasJob *jobs, uint32_t K, hipStream_t s, uint32_t step = 1,
                                uint32_t fused_frames = 0, uint64_t in_stride = 0)
{
	Device &d = *g_context.cur;
	const uint32_t n = route.kernel_views;
	const size_t rows_bytes = sizeof(BfViewRow) * n, table_bytes = rows_bytes + sizeof(uint32_t) * (n + 1);
	bool ok = stage_table(table_bytes, s, [&](void *pinned) {
		BfViewRow *rows = (BfViewRow *)pinned;
		for (uint32_t k = 0, r = 0; k < K; k++) {
			if (!route.taken[k]) continue;
			rows[r] = route.rows[r];
			rows[r].out_offset = (uint64_t)(jobs[k * step].out - jobs[0].out);
			rows[r].out_stride = fused_frames > 1 ? (uint64_t)(jobs[k * step + 1].out - jobs[k * step].out) : 0;
			r++;
		}
		std::memcpy((char *)pinned + rows_bytes, route.first_block.data(), sizeof(uint32_t) * (n + 1));
	});
	BfDasArgs a = route.a;
	a.rf = jobs[0].in; a.out = jobs[0].out;
	bind_tables(ps, a);
	BfViewsArgs v{};
	v.rows = (const BfViewRow *)d.views_table.ptr;
	v.first_block = (const uint32_t *)((const char *)d.views_table.ptr + rows_bytes);
	v.view_count = n;
	BfBurstArgs b{};
	b.frame_count = fused_frames; b.rf_stride = in_stride;
	if (ok) ok &= fused_frames ? HIP_OK(bf_launch_das_burst_views(&a, &b, &v, route.first_block[n], s)) : HIP_OK(bf_launch_das_views(&a, &v, route.first_block[n], s));
	return ok;
}

/* A READI image push's decode across acquisitions (readi_decode.hip): the N DAS inputs at `cur`, cur_stride bytes apart, each
 * [channel][A][samples], into d.readi_decoded (push_frames grew it) as [channel][G x A][samples] by the signs of the block's own READI
 * matrix (ps: the block's plan state -- the table the block's READI kernels read).  `cur` becomes the decoded buffer, decoded_bytes of
 * it what beamformer_hip_copy_das_input serves. */
static bool launch_decode_step(PlanState *ps, const BeamformerParameters &bp, const char *&cur, uint64_t &cur_stride, const uint32_t *groups, uint32_t N,
                                uint64_t decoded_bytes, hipStream_t s)
{
	Device &d = *g_context.cur;
	const Plan &plan = ps->plan;
	bool ok = true;
	if (hooks().scratch_poison) ok &= HIP_OK(hipMemsetAsync(d.readi_decoded.ptr, 0xFF, d.readi_decoded.size, s));
	ok &= stage_group_ids(groups, N, s);
	BfReadiDecodeArgs a{};
	a.in = cur; a.out = d.readi_decoded.ptr;
	a.groups   = (const uint32_t *)d.views_table.ptr;
	a.hadamard = (const uint32_t *)ps->readi_hadamard.ptr;
	a.in_frame_bytes = N > 1 ? cur_stride : 0;
	a.slab_floats = (uint64_t)plan.acquisitions * plan.das_samples * (plan.iq_pipeline ? 2u : 1u);
	a.frames = N; a.group_count = bp.readi_group_count; a.channels = plan.channels;
	ok = ok && HIP_OK(bf_launch_readi_image_decode(&a, s));
	d.das_decoded_bytes = decoded_bytes;
	cur = (const char *)d.readi_decoded.ptr; cur_stride = 0;
	return ok;
}

/* some job that is not fused has a Staged or Tile part: its own launch keeps the per-frame counters -- [0] staged window violations,
 * [1] / [2] das_tile.hip's staged / gathered chunks */
static bool wants_counters(const DasJob *jobs, uint32_t count)
{
	for (uint32_t k = 0; k < count; k++) {
		if (jobs[k].fused || !jobs[k].parts) continue;
		for (const DasDecision &dd : *jobs[k].parts) if (dd.path == DasPath_Staged || dd.path == DasPath_Tile) return true;
	}
	return false;
}

/* The geometry-only recount of job j's apodization test into `mine`: the general kernel's count over every part of the frame. */
static bool launch_pair_count(PlanState *das_ps, const DasJob &j, unsigned long long *mine, uint64_t voxel_bytes, hipStream_t s)
{
	bool ok = HIP_OK(hipMemsetAsync(mine, 0, sizeof(*mine), s));
	const DasDecision &head = main_part(*j.parts);
	for (const DasDecision &dd : *j.parts) {
		if (!ok || dd.path == DasPath_Zero) continue;
		BfDasArgs count = dd.general;              /* the general kernel's own tiles: the specialised kernels reshape them */
		count.rf = j.in; count.out = j.out + (uint64_t)(dd.z_first - j.z_first) * head.a.size[0] * head.a.size[1] * voxel_bytes;
		bind_tables(das_ps, count);
		if (j.group >= 0) count.readi_group = (uint32_t)j.group;
		count.pair_counter = mine;
		ok &= HIP_OK(bf_launch_das_count(&count, s));
	}
	return ok;
}

/* The stages of a plan over one push, in stream order, with one timing segment per stage in w.t.
 * Pre-DAS: every stage ONE launch for all RF frames (launch_stage), ping-ponging between the push's stage buffers.
 * DAS: the push's frames are placed in the ring (next_frames) and each job's `in` -- its RF frame's slice of the DAS input -- and `out`
 * -- its ring slot -- resolved.  Then, in this order: the optional decode step, which replaces the DAS input; the push's fused launch
 * for the jobs marked `fused`, dispatched by kind in the one switch below; every other job's own launch(es), the kernels of a single
 * push; the pair count, once per run of jobs with the same parts.  Which push is running shows in that switch and nowhere else: all
 * other steps read the job list.
 * No DAS stage in the plan: the frames are placed and cleared.  Last, the DAS fields of every frame's timing row. */
static bool walk_plan(uint32_t block, PlanState *ps, const Push &w)
{
	Context &c = g_context;
	Device  &d = *c.cur;
	const Plan &plan = ps->plan;
	const ParameterBlock &pb = c.blocks[block];
	hipStream_t s = d.stream;
	TimingSlot &t = *w.t;
	const uint32_t N = w.rf_frames, F = w.frames;
	DasJob *jobs = w.jobs;

	const char *cur = (const char *)w.in;
	uint64_t cur_stride = w.in_stride;
	int64_t  cur_bound = w.in_bound;
	int toggle = 0;
	bool ok = true;
	d.das_input = nullptr; d.das_input_bytes = d.das_input_stride = 0; d.das_input_frames = 0; d.das_decoded_bytes = 0;

	const uint64_t voxel_bytes = plan.iq_pipeline ? 8u : 4u;
	const uint64_t first = d.frame_counter;                 /* the id of the walk's first frame */
	const bool counters_kept = wants_counters(jobs, F);

	/* hook SCRATCH_POISON: both intermediate buffers, and below the frames' ring slots once next_frames has placed them (nothing writes
	 * them before the DAS stage), are filled with 0xFF bytes -- NaN in binary16 and in f32 -- so that an element a stage reads without
	 * this push having written it shows up as NaN.  Unset: no memset, no launch. */
	const bool poison = hooks().scratch_poison;
	if (poison)
		for (int k = 0; k < 2; k++)
			if (w.stage[k].ptr) ok &= HIP_OK(hipMemsetAsync(w.stage[k].ptr, 0xFF, w.stage[k].size, s));

	for (size_t i = 0; i < plan.stages.size() && ok; i++) {
		const Stage &st = plan.stages[i];
		bool das_segment_done = false;
		switch (st.kind) {
		case BeamformerShaderKind_Reshape:
		case BeamformerShaderKind_Decode:
		case BeamformerShaderKind_Hilbert:
		case BeamformerShaderKind_Filter:
		case BeamformerShaderKind_Demodulate:{
			DeviceBuffer &out = w.stage[toggle];
			/* What the next stage may read of this one's output is what the plan's stages can write of a buffer, plan.intermediate_bytes --
			 * not the allocation, which a larger plan may have grown and filled.  Filter and Demodulate read windows of consecutive
			 * elements wherever their row starts put them (filter.glsl:81-87 halves a row start): below that bound they reach elements this
			 * stage does not write -- the second half of every row of a root-layout buffer after demodulation, the bytes behind a
			 * narrower kind's extent.  The reference never clears its ping-pong buffer (beamformer_core.c:1229-1237) and finds there what
			 * the stage two hops back, or an earlier frame, left in the slot.  This build defines such elements as zero: the buffer is
			 * cleared first wherever the stage does not write all of it (the oracle clears its slots the same way, oracle_plan.c). */
			const Stage *next = i + 1 < plan.stages.size() ? &plan.stages[i + 1] : nullptr;
			if (next && (next->kind == BeamformerShaderKind_Filter || next->kind == BeamformerShaderKind_Demodulate)) {
				uint64_t dense = (uint64_t)plan.das_samples * plan.channels * plan.acquisitions * (uint64_t)bf_kind_byte_size[st.out_kind];
				if (bf_kind_complex[st.in_kind] && !bf_kind_complex[st.out_kind] &&
				    (st.kind == BeamformerShaderKind_Filter || st.kind == BeamformerShaderKind_Demodulate)) dense *= 2;
				if (dense != plan.intermediate_bytes)
					ok &= HIP_OK(hipMemsetAsync(out.ptr, 0, w.stage_stride ? w.stage_stride * N : plan.intermediate_bytes, s));
			}
			ok &= launch_stage(ps, pb.parameters, i, cur, cur_bound, out.ptr, s, N, cur_stride, w.stage_stride);
			cur = (const char *)out.ptr; cur_stride = w.stage_stride; cur_bound = (int64_t)plan.intermediate_bytes; toggle ^= 1;
		}break;
		case BeamformerShaderKind_DAS:{
			uint64_t run_bytes = 0;
			FrameRecord *frame0 = next_frames(jobs, F, plan.iq_pipeline, block, run_bytes);
			if (!frame0) return set_error(BeamformerLibErrorKind_FrameSizeOverflow);
			if (poison && run_bytes) ok &= HIP_OK(hipMemsetAsync((char *)d.ring.ptr + frame0->offset, 0xFF, run_bytes, s));
			/* what beamformer_hip_copy_das_input_frame serves: RF frame k's input at k * cur_stride (one RF frame: all jobs share the one
			 * input) */
			d.das_input = cur; d.das_input_bytes = (uint64_t)plan.das_samples * plan.acquisitions * plan.channels * voxel_bytes;   /* [channel][transmit][sample] */
			d.das_input_stride = N > 1 ? cur_stride : 0; d.das_input_frames = N;
			/* (Flag 0x2000: the step fails here, as a refused launch would -- the only way to such a push's tombstones that needs no
			 * device fault: everything a caller can get wrong is refused before the ids are taken) */
			if (w.fails_on_flag && (c.das_path_mode & BeamformerHipDasPath_FailViewsDas)) return set_error(BeamformerLibErrorKind_InvalidAccess);
			if (!jobs[0].parts) break;   /* more devices than planes: this device holds an empty slab of the frame */

			/* ---- the jobs.  Which kernel, with which geometry: the ladder of rules of decide_das (das_select.cpp), in each job's parts.  Usually ONE
			 * launch per job; where a term of the frame can reach an end of its RF row the z range is cut and the planes concerned go to
			 * the kernel behind the staged one (decide_das_parts, das_exact.h). */
			if (w.decode_groups && main_part(*jobs[0].parts).path != DasPath_Zero) {
				/* ---- 0. the decode step, its own segment directly before DAS */
				ok &= launch_decode_step(ps, pb.parameters, cur, cur_stride, w.decode_groups, N, main_part(*jobs[0].parts).das_input_bytes, s);
				segment(t, (uint32_t)BeamformerShaderKind_Decode, s);
			}
			bool any_fused = false, any_counted = false;
			for (uint32_t k = 0; k < F; k++) {
				DasJob &j = jobs[k];
				j.in  = cur + j.rf_frame * cur_stride;
				j.out = (char *)d.ring.ptr + d.frames[(first + k) % d.frames.size()].offset;
				const DasDecision &head = main_part(*j.parts);
				j.path = (uint32_t)(head.path == DasPath_Zero ? DasPath_General : head.path);
				any_fused   |= j.fused;
				any_counted |= head.path != DasPath_Zero;
			}

			/* ---- 1. the push's fused launch.  Jobs are view-major where there are views: view v's RF frame k is job v * N + k */
			switch (any_fused ? w.fused.kind : FusedLaunch::None) {
			case FusedLaunch::None:       break;
			case FusedLaunch::Burst:      ok &= launch_burst_kernel(ps, *w.fused.burst, jobs[0], nullptr, N, cur_stride, frame0->bytes, s); break;
			case FusedLaunch::ReadiSweep: ok &= launch_burst_kernel(ps, *w.fused.burst, jobs[0], w.fused.groups, N, cur_stride, frame0->bytes, s); break;
			case FusedLaunch::Views:      ok &= launch_views_kernel(ps, *w.fused.views, jobs, F, s); break;
			case FusedLaunch::Variants:   ok &= launch_variants_kernel(ps, *w.fused.variants, jobs, F, s); break;
			case FusedLaunch::BurstViews: ok &= launch_views_kernel(ps, *w.fused.views, jobs, F / N, s, N, N, N > 1 ? cur_stride : 0); break;
			case FusedLaunch::ViewsPerRfFrame:      /* RF frame k: jobs k, N + k, 2 N + k, ... */
				for (uint32_t k = 0; k < N && ok; k++) ok &= launch_views_kernel(ps, *w.fused.views, jobs + k, F / N, s, N);
				break;
			}
			/* ---- 2. every other job's own launch(es): the kernels of a single push.  One set of counters per timing slot */
			if (counters_kept && !d.staged_violations.ensure(sizeof(uint32_t) * 4 * kTimingSlots)) ok = false;
			for (uint32_t k = 0; k < F && ok; k++) {
				DasJob &j = jobs[k];
				if (j.fused) continue;
				uint32_t *frame_counters = nullptr;
				if (counters_kept && F - k <= kTimingSlots) {        /* the table keeps the newest 32 frames: older ones of a long push count nothing */
					frame_counters = (uint32_t *)d.staged_violations.ptr + 4 * ((first + k) % kTimingSlots);
					ok &= HIP_OK(hipMemsetAsync(frame_counters, 0, 4 * sizeof(uint32_t), s));
				}
				const DasDecision &head = main_part(*j.parts);
				ok &= launch_frame_parts(w.das_ps, *j.parts, j.z_first, (uint64_t)head.a.size[0] * head.a.size[1] * voxel_bytes, j.in, j.out, frame_counters, s, j.path, j.group);
			}
			/* ---- 3. geometry-only recount of the apodization test; its own segment so that it stays out of the DAS time.  The count is
			 * the same for every job of a run of jobs with the same parts (jobs that differ in their group alone are one run: the group
			 * only signs the terms; jobs under different f-numbers are not): it runs once, into the counter of the run's last frame, and
			 * the run's other frames' counters are copies -- the newest 32 frames only */
			if (c.count_pairs && any_counted) {
				segment(t, (uint32_t)st.kind, s);
				ok &= d.pair_counter.ensure(sizeof(unsigned long long) * (kTimingSlots + 2));
				unsigned long long *counters = (unsigned long long *)d.pair_counter.ptr;
				for (uint32_t begin = 0, end; begin < F && ok; begin = end) {
					for (end = begin + 1; end < F && jobs[end].parts == jobs[begin].parts; end++) {}
					if (F - (end - 1) > kTimingSlots) continue;
					unsigned long long *mine = counters + (first + end - 1) % kTimingSlots;
					ok &= launch_pair_count(w.das_ps, jobs[begin], mine, voxel_bytes, s);
					for (uint32_t k = end - 1; k-- > begin && F - k <= kTimingSlots && ok;)
						ok &= HIP_OK(hipMemcpyAsync(counters + (first + k) % kTimingSlots, mine, sizeof(*mine), hipMemcpyDeviceToDevice, s));
				}
				segment(t, kStagePairCount, s);
				t.counted = true;
				das_segment_done = true;
			}
		}break;
		default: break;      /* CoherencyWeighting: fused into the DAS epilogue (das.hip); kept in the plan so that the stage list a client
		                      * sees through beamformer_compute_timings matches the reference's */
		}
		if (!das_segment_done) segment(t, (uint32_t)st.kind, s);
	}
	if (plan.das_index < 0 && ok) {
		/* no DAS in the pipeline: the frames exist and stay zero (the reference clears them, beamformer_core.c:1573-1585, and nothing
		 * writes them) */
		uint64_t run_bytes = 0;
		FrameRecord *frame0 = next_frames(jobs, F, plan.iq_pipeline, block, run_bytes);
		if (!frame0) return set_error(BeamformerLibErrorKind_FrameSizeOverflow);
		if (run_bytes) ok &= HIP_OK(hipMemsetAsync((char *)d.ring.ptr + frame0->offset, 0, run_bytes, s));
	}
	if (!ok) return set_error(BeamformerLibErrorKind_InvalidAccess);
	for (uint32_t k = 0; k < F; k++) {
		const bool own_counters = counters_kept && F - k <= kTimingSlots;
		const DasJob &j = jobs[k];                            /* parts null: no DAS kernel ran for the frame */
		fill_das_fields(d.timing[(first + k) % kTimingSlots], first + k, j.parts, j.points, plan.iq_pipeline, j.path, own_counters ? (first + k) % kTimingSlots : ~0ull);
	}
	return true;
}

/* One frame of a single push: the walk over d.scratch[], timed in the frame's own slot, with its one job on the stack. */
static bool run_frame_stages(uint32_t block, const void *rf, int64_t rf_bytes, bool ingest_timed)
{
	Context &c = g_context;
	Device &d = *c.cur;
	PlanState *ps = commit_block(block);
	if (!ps) return set_error(BeamformerLibErrorKind_InvalidComputeStage);
	const Plan &plan = ps->plan;
	const ParameterBlock &pb = c.blocks[block];
	TimingSlot &t = d.timing[d.frame_counter % kTimingSlots];
	t.failed = false; t.share = 1;
	if (!ensure_events(t)) return false;
	/* events[0] was recorded in front of the ingest by the caller when ingest_timed */
	t.count = 0; t.counted = false;
	if (ingest_timed) segment(t, kStageIngest, d.stream);
	else              record(t, 0, d.stream);

	uint32_t zfirst, zcount;
	shard_planes(pb, plan, zfirst, zcount);
	if (c.device_count > 1) { zfirst = d.slab_first; zcount = d.slab_count; }   /* this device's z-slab (run_peers) */
	/* no DAS in the pipeline: a single push's frame is the block's whole grid whatever its shard -- with several devices on the ingest
	 * device, the others holding an empty slab of it (a burst's frames are the shard's planes) */
	if (plan.das_index < 0) zcount = c.device_count > 1 && d.index != 0 ? 0u : plan.output_points[2];
	const uint32_t points[3] = {plan.output_points[0], plan.output_points[1], zcount};
	DasJob one{};
	one.points = points; one.z_first = zfirst; one.group = -1;
	one.parts = frame_das_parts(ps, pb, zfirst, zcount);
	Push w;
	w.in = rf; w.in_bound = rf_bytes; w.stage = d.scratch; w.t = &t;
	w.jobs = &one; w.das_ps = ps;
	return walk_plan(block, ps, w);
}

/* z-slab of device `i` of `n` over `planes` planes starting at `first`: contiguous, sizes differing by
 * at most one -- the rule of ogl_beamforming_amd/sharding.py (one process per GPU), so both ways of
 * spreading a frame over a node cut it at the same planes */
static void device_slab(uint32_t i, uint32_t n, uint32_t first, uint32_t planes, uint32_t &z_first, uint32_t &z_count)
{
	uint32_t begin = (uint32_t)((uint64_t)i * planes / n), end = (uint32_t)((uint64_t)(i + 1) * planes / n);
	z_first = first + begin;
	z_count = end - begin;
}

/* Several devices, one frame: the channel-mapped RF that the ingest device (devices[0])
 * holds at `src` is copied to every peer's RF slot -- hipMemcpyPeerAsync, one stream per destination, so
 * the copies run side by side on their xGMI links and, three RF slots deep, beside the kernels of the
 * previous frame -- and every peer beamforms its own z-slab of the block's grid.  No reduction
 * collective: voxels are independent.  Called with devices[0] current and its ingest already
 * enqueued on its stream; returns with devices[0] current again. */
static bool run_peers(uint32_t block, const void *src, uint64_t rf_size, uint32_t slot)
{
	Context &c = g_context;
	Device  &d0 = c.devices[0];
	const ParameterBlock &pb = c.blocks[block];
	const uint32_t n = c.device_count;
	const uint32_t planes_total = (uint32_t)(pb.parameters.output_points[2] > 1 ? pb.parameters.output_points[2] : 1);
	const uint32_t first  = pb.shard_z_count ? pb.shard_z_first : 0u;
	const uint32_t planes = pb.shard_z_count ? pb.shard_z_count : planes_total;
	for (uint32_t i = 0; i < n; i++) device_slab(i, n, first, planes, c.devices[i].slab_first, c.devices[i].slab_count);

	/* "the mapped RF of this frame is complete on the ingest device" */
	bool ok = HIP_OK(hipEventRecord(d0.rf_landed[slot], d0.stream));
	for (uint32_t i = 1; i < n && ok; i++) {
		Device &p = c.devices[i];
		if (!select_device(i)) { ok = false; break; }
		ok &= p.rf[slot].ensure(round_up(rf_size, 64) + 64);
		ok &= HIP_OK(hipStreamWaitEvent(p.peer_stream, d0.rf_landed[slot], 0));
		/* the frame that read this slot three pushes ago must be done with it */
		if (p.consumed_pending[slot]) ok &= HIP_OK(hipStreamWaitEvent(p.peer_stream, p.rf_consumed[slot], 0));
		if (!ok) break;
		ok &= HIP_OK(hipEventRecord(p.peer_copy_begin[slot], p.peer_stream));
		ok &= HIP_OK(hipMemcpyPeerAsync(p.rf[slot].ptr, p.device, src, d0.device, rf_size, p.peer_stream));
		ok &= HIP_OK(hipEventRecord(p.peer_copy_end[slot], p.peer_stream));
		ok &= HIP_OK(hipEventRecord(p.rf_landed[slot], p.peer_stream));
		p.last_rf = p.rf[slot].ptr; p.last_rf_bytes = rf_size; p.last_rf_slot = slot;
		ok &= HIP_OK(hipStreamWaitEvent(p.stream, p.rf_landed[slot], 0));
		TimingSlot &t = p.timing[p.frame_counter % kTimingSlots];
		t.sampled = true; t.failed = false; t.events_slot = (uint32_t)(p.frame_counter % kTimingSlots);
		ok = ok && run_frame(block, p.rf[slot].ptr, (int64_t)rf_size, false);
		p.consumed_pending[slot] = ok && HIP_OK(hipEventRecord(p.rf_consumed[slot], p.stream));
	}
	if (!select_device(0)) ok = false;
	return ok || set_error(BeamformerLibErrorKind_InvalidAccess);
}

/* The pinned slot of an upload, free again (the copy or kernel that last read it has finished) and at least `size` bytes. */
static bool claim_pinned(UploadSlot &u, uint64_t size)
{
	if (u.copy_pending) { (void)hipEventSynchronize(u.copied); u.copy_pending = false; }
	if (u.pinned_size >= size) return true;
	if (u.pinned) (void)hipHostFree(u.pinned);
	u.pinned = nullptr; u.pinned_size = 0;
	if (!HIP_OK(hipHostMalloc(&u.pinned, round_up(size, 4096), hipHostMallocDefault))) {
		u.pinned = nullptr; (void)hipGetLastError();
		return false;
	}
	u.pinned_size = round_up(size, 4096);
	return true;
}

/* The caller's bytes into a pinned slot.  One core copies ~37 GB/s into pinned memory here; copies of 64 MiB and more are split over a few
 * short-lived threads (the copy of a 512 MiB decode-benchmark frame drops from 14 ms to what the memory system gives). */
static void copy_to_pinned(void *pinned, const void *data, size_t size)
{
	constexpr size_t kParallelCopyBytes = 64u << 20;
	if (size < kParallelCopyBytes) { std::memcpy(pinned, data, size); return; }
	const unsigned parts = 4;
	const size_t   piece = ((size + parts - 1) / parts + 4095) & ~(size_t)4095;
	std::thread workers[parts - 1];
	for (unsigned i = 1; i < parts; i++) {
		size_t begin = piece * i, end = begin + piece < size ? begin + piece : size;
		workers[i - 1] = std::thread([=] { if (begin < end) std::memcpy((char *)pinned + begin, (const char *)data + begin, end - begin); });
	}
	std::memcpy(pinned, data, piece < size ? piece : size);
	for (auto &w : workers) w.join();
}

/* How a push's RF lies in the caller's buffer (rows of in_row bytes, one per raw channel) and in the RF ring (rows of out_row bytes, one
 * per mapped channel; rf_size per frame). */
struct RfLayout {
	uint64_t in_row, out_row, rf_size;
	bool     a1s2, identity;        /* identity: channel_mapping[ch] == ch for every channel */
};

static bool rf_layout(const ParameterBlock &pb, RfLayout &l)
{
	const BeamformerParameters &bp = pb.parameters;
	const uint64_t bytes = (uint64_t)bf_kind_byte_size[pb.data_kind];
	l.out_row = bytes * bp.sample_count * bp.acquisition_count;
	l.in_row  = bytes * bp.raw_data_dimensions[0];
	l.rf_size = l.out_row * bp.channel_count;
	/* the reference copies whatever row the mapping names (lib .c:520-528); on a GPU an
	 * out-of-range row would fault, so it is an error here */
	l.identity = true;
	for (uint32_t ch = 0; ch < bp.channel_count; ch++) {
		uint16_t row = (uint16_t)pb.channel_mapping[ch];
		if (row >= bp.raw_data_dimensions[1]) return set_error(BeamformerLibErrorKind_DataSizeMismatch);
		l.identity &= row == ch;
	}
	l.a1s2 = bp.contrast_mode == BeamformerContrastMode_A1S2;
	return true;
}

/* How a push's RF reaches the RF ring: the ONE rule, followed by push_rf_and_compute and push_frames and reported by
 * beamformer_hip_describe_upload (include/ogl_beamformer_hip.h names the routes).  Host arithmetic only.
 *   direct     the mapped layout is the raw layout, so one copy (H2D or D2D) lands the RF in its slot and no ingest kernel runs --
 *              unless the upload is small, when the ingest kernel IS the copy out of the pinned slot.  A single push only: a push of
 *              several frames (and the views and variants pushes of one) always runs the ingest kernel;
 *   overlap    host data of kOverlapBytes and more, all frames together: H2D on the copy stream;
 *   zero_copy  other host data: the ingest kernel reads the pinned slot in place;
 *   borrowed   device-resident RF already in the mapped layout is read in place by the first stage (no copy into the RF ring): the
 *              caller keeps it unchanged until the frame has run, which stream order gives for free when its producer is on the
 *              library's stream.  Plans that start with DAS still copy: the DAS input needs the library's zero block behind it. */
struct UploadDecision {
	uint32_t route;                         /* BeamformerHipUploadRoute */
	bool     direct, overlap, zero_copy, borrowed, ingest;
	uint32_t ingest_kernel, copy_bytes;     /* 0 none, 1 copy (copy_bytes per lane and step, for buffers of the library's own), 2 A1S2 */
	uint64_t in_step, rf_step;              /* several frames: frame k of the raw data and of the RF slot at k times these */
};

static UploadDecision decide_upload(const RfLayout &l, const Plan &plan, uint64_t frame_size, uint32_t frames, bool multi_frame_push,
                                    const void *device_pointer)
{
	UploadDecision u{};
	const bool on_device = device_pointer != nullptr;
	u.direct    = !multi_frame_push && l.identity && !l.a1s2 && l.in_row == l.out_row;
	u.overlap   = !on_device && frame_size * frames >= kOverlapBytes;
	u.zero_copy = !on_device && !u.overlap;
	u.borrowed  = on_device && u.direct && !plan.stages.empty() && plan.stages[0].kind != BeamformerShaderKind_DAS;
	u.ingest    = !u.direct || u.zero_copy;
	if (on_device) u.route = u.borrowed ? BeamformerHipUploadRoute_DeviceBorrowed : u.ingest ? BeamformerHipUploadRoute_DeviceIngest : BeamformerHipUploadRoute_DeviceCopy;
	else           u.route = u.zero_copy ? BeamformerHipUploadRoute_PinnedInPlace : u.ingest ? BeamformerHipUploadRoute_CopyEngineStaged : BeamformerHipUploadRoute_CopyEngineDirect;
	u.in_step = frames > 1 ? frame_size : 0;
	u.rf_step = frames > 1 ? round_up(l.rf_size, 64) + 64 : 0;
	u.ingest_kernel = !u.ingest ? 0u : l.a1s2 ? 2u : 1u;
	u.copy_bytes = u.ingest_kernel == 1 ? bf_ingest_copy_bytes(l.in_row, l.out_row, (uint64_t)(uintptr_t)device_pointer, 0, u.in_step, u.rf_step) : 0u;
	return u;
}

bool describe_upload(const ParameterBlock &pb, const Plan &plan, uint64_t frame_size, uint32_t frames, const void *device_pointer,
                     BeamformerHipUploadDescription *out)
{
	static const char *const names[BeamformerHipUploadRoute_Count] = {"pinned-in-place", "copy-engine-direct", "copy-engine-staged",
	                                                                  "device-borrowed", "device-copy", "device-ingest"};
	RfLayout l;
	if (!rf_layout(pb, l)) return false;
	const UploadDecision u = decide_upload(l, plan, frame_size, frames, frames > 1, device_pointer);
	std::memset(out, 0, sizeof(*out));
	out->route = u.route; out->ingest_kernel = u.ingest_kernel; out->copy_bytes = u.copy_bytes;
	out->a1s2_base = (uint32_t)bf_kind_base[pb.data_kind];
	out->rf_bytes = l.rf_size; out->upload_bytes = frame_size * frames;
	std::snprintf(out->name, sizeof(out->name), "%s", names[u.route]);
	return true;
}

/* The ingest kernel: `frames` raw frames at `raw` into the mapped layout at `out`, frame k at k * the frame strides (one frame: 0). */
static bool launch_ingest(PlanState *ps, const ParameterBlock &pb, const RfLayout &l, const void *raw, void *out, uint32_t frames,
                          uint64_t in_frame_bytes, uint64_t out_frame_bytes, hipStream_t s)
{
	BfIngestArgs a{};
	a.raw = raw; a.out = out;
	a.channel_mapping = (const int16_t *)ps->mapping.ptr;
	a.in_row_bytes = l.in_row; a.out_row_bytes = l.out_row; a.channels = pb.parameters.channel_count;
	a.a1s2 = l.a1s2; a.base = bf_kind_base[pb.data_kind];
	a.a1s2_scalars = pb.parameters.sample_count * (uint32_t)bf_kind_element_count[pb.data_kind];
	a.frames = frames; a.in_frame_bytes = in_frame_bytes; a.out_frame_bytes = out_frame_bytes;
	return HIP_OK(bf_launch_ingest(&a, s));
}

/* The upload of a push's host bytes, in the three steps a burst needs apart (it grows every buffer before it takes its ids):
 *   claim_upload     the slot's events exist and -- host data -- its pinned memory is free and large enough;
 *   enqueue_upload   the caller's bytes are copied into the pinned slot (after which the caller may reuse its buffer, as with the
 *                    reference's copy into shared memory).  With a device destination the H2D runs on the copy stream and the compute
 *                    stream waits for it -- so the upload of push n+1 overlaps the kernels of push n, which one stream and pageable
 *                    memory cannot do; without one (uploads under kOverlapBytes) the first kernel reads the pinned slot in place.
 *                    Returns what that kernel reads, or null;
 *   pinned_read_by / finish_upload   the fences the next user of the slot waits on. */
static bool claim_upload(UploadSlot &u, uint64_t size, bool host_data)
{
	if (!u.copied && (!HIP_OK(hipEventCreateWithFlags(&u.copied, hipEventDisableTiming)) ||
	                  !HIP_OK(hipEventCreateWithFlags(&u.consumed, hipEventDisableTiming))))
		return set_error(BeamformerLibErrorKind_SharedMemory);
	if (host_data && !claim_pinned(u, size)) return set_error(BeamformerLibErrorKind_BufferOverflow);
	return true;
}

static const void *enqueue_upload(Device &d, UploadSlot &u, const void *data, uint64_t size, void *dst, uint64_t dst_bytes)
{
	hipStream_t s = d.stream;
	copy_to_pinned(u.pinned, data, size);
	void *mapped = nullptr;
	if (!dst) return HIP_OK(hipHostGetDevicePointer(&mapped, u.pinned, 0)) ? mapped : nullptr;
	bool ok = true;
	/* the device buffers of this slot were last read by the push three pushes ago; if that
	 * push recorded no `consumed` event (small or device-resident pushes do not), fence
	 * against everything enqueued so far instead */
	if (u.unfenced_reader) { u.consume_pending = HIP_OK(hipEventRecord(u.consumed, s)); u.unfenced_reader = false; }
	if (u.consume_pending) ok &= HIP_OK(hipStreamWaitEvent(d.copy_stream, u.consumed, 0));
	ok &= HIP_OK(hipMemcpyAsync(dst, u.pinned, dst_bytes, hipMemcpyHostToDevice, d.copy_stream));
	ok &= HIP_OK(hipEventRecord(u.copied, d.copy_stream));
	u.copy_pending = true;
	ok &= HIP_OK(hipStreamWaitEvent(s, u.copied, 0));
	return ok ? dst : nullptr;
}

/* the kernel just enqueued on s read the pinned slot in place: the slot is free again once it has run */
static bool pinned_read_by(UploadSlot &u, hipStream_t s)
{
	u.copy_pending = true;
	return HIP_OK(hipEventRecord(u.copied, s));
}

/* after the push's last launch: a push that went over the copy engine records `consumed`, any other leaves an unfenced reader */
static void finish_upload(UploadSlot &u, bool overlap, hipStream_t s)
{
	if (overlap) { u.consume_pending = HIP_OK(hipEventRecord(u.consumed, s)); u.unfenced_reader = false; }
	else         { u.consume_pending = false; u.unfenced_reader = true; }
}

static void note_push_time()
{
	Context &c = g_context;
	double now = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
	if (c.last_push_time > 0) {
		if (c.rf_time_deltas.size() >= 32) c.rf_time_deltas.erase(c.rf_time_deltas.begin());
		c.rf_time_deltas.push_back((float)(now - c.last_push_time));
	}
	c.last_push_time = now;
}

/* A push owns ids [first, first + count) on the first device_count devices (a single push: one id on every device of the set; a burst:
 * count ids on one device).  Whatever fails after the ids are taken -- a peer's replan, a peer copy, the stages -- the next push starts
 * all devices on the same id again, and a push that does not complete leaves a TOMBSTONE under each of its ids (no bytes, no voxels, no
 * stage timings): the readers below refuse it -- "the newest frame is missing" -- instead of serving whatever record sat in that ring
 * slot BeamformerMaxBacklogFrames pushes ago. */
struct Tombstones {
	Context &c; uint64_t first; uint32_t count, device_count; bool complete;
	~Tombstones() {
		for (uint32_t i = 0; i < device_count; i++) {
			Device &p = c.devices[i];
			p.frame_counter = first + count;
			if (complete) continue;
			for (uint64_t id = first; id < first + count; id++) {
				FrameRecord &f = p.frames[id % p.frames.size()];
				f = FrameRecord{}; f.points[0] = f.points[1] = f.points[2] = 0; f.id = (uint32_t)id; f.failed = true;
				TimingSlot &t = p.timing[id % kTimingSlots];
				t.count = 0; t.counted = false; t.violations_slot = ~0ull; t.das_voxels = 0; t.frame_id = id; t.failed = true;
			}
		}
	}
};

/* lib .c:491-570 (client copy) + beamformer_core.c:1756-1805 (upload worker) */
bool push_rf_and_compute(uint32_t block, const void *data, uint32_t size, bool data_on_device)
{
	Context &c = g_context;
	Device  &d = *c.cur;
	ParameterBlock &pb = c.blocks[block];
	const BeamformerParameters &bp = pb.parameters;
	hipStream_t s = d.stream;

	RfLayout l;
	if (!rf_layout(pb, l)) return false;
	const uint64_t rf_size = l.rf_size;

	uint32_t slot = (uint32_t)(d.rf_index++ % BeamformerMaxRawDataFramesInFlight);
	if (!d.rf[slot].ensure(round_up(rf_size, 64) + 64)) return set_error(BeamformerLibErrorKind_RFDataSizeOverflow);
	const bool multi = c.device_count > 1;
	/* ONE frame id for every device of the set, taken here -- before the plan is committed: a push refused from here on leaves a tombstone */
	const uint64_t sequence = c.push_sequence++;
	for (uint32_t i = 0; i < c.device_count; i++) c.devices[i].frame_counter = sequence;
	Tombstones lockstep{c, sequence, 1, c.device_count, false};
	if (multi) {
		/* every peer replans before the ingest device does (its commit clears the dirty bits) */
		for (uint32_t i = 1; i < c.device_count; i++) {
			if (!select_device(i) || !commit_block(block)) { select_device(0); return set_error(BeamformerLibErrorKind_InvalidComputeStage); }
		}
		if (!select_device(0)) return set_error(BeamformerLibErrorKind_SharedMemory);
		/* this RF slot was the source of the peer copies three pushes ago: they must have landed before
		 * anything overwrites it (long done by now; waiting on a never-recorded event is a no-op) */
		for (uint32_t i = 1; i < c.device_count; i++) {
			(void)hipStreamWaitEvent(s, c.devices[i].rf_landed[slot], 0);
			(void)hipStreamWaitEvent(d.copy_stream, c.devices[i].rf_landed[slot], 0);
		}
	}

	TimingSlot &t = d.timing[d.frame_counter % kTimingSlots];
	t.failed = false;
	if (!ensure_events(t)) return false;
	/* sample this frame's per-stage timings?  always for frames that are not small, after a replan,
	 * when pair counting rides along, and every kTimingSamplePeriod-th frame otherwise */
	const bool small = rf_size < kSmallFrameBytes &&
	                   (uint64_t)bp.output_points[0] * (uint64_t)(bp.output_points[1] > 1 ? bp.output_points[1] : 1) *
	                   (uint64_t)(bp.output_points[2] > 1 ? bp.output_points[2] : 1) < (4ull << 20);
	if (!d.have_sample || pb.dirty != 0 || block != d.last_sampled_block) d.replan_frame = d.frame_counter;
	/* the first frames of a plan are all sampled: the very first carries one-off launch costs */
	t.sampled = !small || c.count_pairs || d.frame_counter - d.replan_frame < 3 ||
	            d.frame_counter - d.last_sampled_frame >= kTimingSamplePeriod;
	if (t.sampled) {
		d.have_sample = true; d.last_sampled_frame = d.frame_counter; d.last_sampled_block = block;
		t.events_slot = (uint32_t)(d.frame_counter % kTimingSlots);
		(void)hipEventRecord(t.events[0], s);
	} else {
		t.events_slot = (uint32_t)(d.last_sampled_frame % kTimingSlots);
	}

	/* the route of a single push: decide_upload */
	UploadSlot &u = d.upload[slot];
	if (!claim_upload(u, size, !data_on_device)) return false;
	PlanState *ps = commit_block(block);
	if (!ps) return set_error(BeamformerLibErrorKind_InvalidComputeStage);
	const UploadDecision route = decide_upload(l, ps->plan, size, 1, false, data_on_device ? data : nullptr);
	const bool overlap = route.overlap, borrowed = route.borrowed;
	const void *raw = data;
	if (!data_on_device) {
		void *dst = nullptr;
		if (overlap) {
			dst = d.rf[slot].ptr;
			if (route.ingest) {
				if (!d.raw_staging[slot].ensure(round_up(size, 64) + 64)) return set_error(BeamformerLibErrorKind_BufferOverflow);
				dst = d.raw_staging[slot].ptr;
			}
		}
		raw = enqueue_upload(d, u, data, size, dst, route.ingest ? (uint64_t)size : rf_size);
		if (!raw) return set_error(BeamformerLibErrorKind_InvalidAccess);
	}
	bool ok = true;
	if (route.ingest) {
		ok &= launch_ingest(ps, pb, l, raw, d.rf[slot].ptr, 1, 0, 0, s);
		if (route.zero_copy) ok &= pinned_read_by(u, s);
	} else if (route.route == BeamformerHipUploadRoute_DeviceCopy) {
		ok &= HIP_OK(hipMemcpyAsync(d.rf[slot].ptr, data, rf_size, hipMemcpyDeviceToDevice, s));
	}
	if (!ok) return set_error(BeamformerLibErrorKind_InvalidAccess);
	note_push_time();

	/* what beamformer_hip_get_device_info checksums later.  A caller's device buffer is only borrowed for the duration of the frame: its
	 * pointer is NOT kept -- with several devices the checksum of what the ingest device read is taken here, on the stream, while the
	 * buffer is guaranteed live; with one device a borrowed frame reports no checksum */
	d.last_rf = borrowed ? nullptr : d.rf[slot].ptr; d.last_rf_bytes = rf_size; d.last_rf_slot = slot; d.last_rf_sum_ready = false;
	if (multi && borrowed && d.pair_counter.ensure(sizeof(unsigned long long) * (kTimingSlots + 2)))
		d.last_rf_sum_ready = HIP_OK(bf_launch_rf_checksum(data, rf_size, (unsigned long long *)d.pair_counter.ptr + kTimingSlots + 1, s));
	if (multi && !run_peers(block, borrowed ? data : d.rf[slot].ptr, rf_size, slot)) return false;
	/* what the first stage may read: this frame's RF -- not the whole RF slot, which behind it holds what a larger frame of three pushes
	 * ago left there (a first stage that indexes past its RF -- the Reshape of a Decode-first pipeline that also demodulates -- reads
	 * zeros, the same in every slot of the ring) */
	bool done = run_frame(block, borrowed ? data : d.rf[slot].ptr, (int64_t)rf_size, true);
	finish_upload(u, overlap, s);
	/* a caller's device buffer read in place: the contract lets the caller overwrite it from work enqueued
	 * later on the library's stream, so that stream also waits for the peer copies out of it */
	if (multi && borrowed)
		for (uint32_t i = 1; i < c.device_count; i++) (void)hipStreamWaitEvent(s, c.devices[i].rf_landed[slot], 0);
	lockstep.complete = done;
	return done;
}

/* Every frame's row of the timing table after a push of N frames with ONE event set, in slot `owner`: the push's events, shared -- each
 * row reports 1 / N of every stage time. */
static void share_timing_rows(Device &d, uint64_t first, uint32_t N, uint32_t owner)
{
	const TimingSlot push = d.timing[owner];
	for (uint32_t k = 0; k < N; k++) {
		const uint64_t id = first + k;
		TimingSlot &ft = d.timing[id % kTimingSlots];
		ft.count = push.count; ft.counted = push.counted;
		std::memcpy(ft.kinds, push.kinds, sizeof(ft.kinds));
		ft.sampled = id % kTimingSlots == owner; ft.events_slot = owner; ft.share = N; ft.failed = false;
	}
	/* older unsampled frames whose row borrowed the events of the slot the push has taken over: their row goes blank rather than show
	 * the push's times as one frame's */
	for (uint32_t k = 0; k < kTimingSlots; k++) {
		TimingSlot &old = d.timing[k];
		if (old.frame_id < first && !old.sampled && old.events_slot == owner) old.count = 0;
	}
}

/* What every multi-frame push starts from: how the block's RF lies in memory, its committed plan, and the planes and grid of its frames
 * (the block's output shard, where it has one).  whole_grid: the push takes one device and no output shard -- its frames are views of
 * their own or cover the block's whole grid -- and is refused otherwise. */
struct PushGround {
	RfLayout   l;
	PlanState *ps;
	uint32_t   z_first, z_count, points[3];
};

static bool begin_push(uint32_t block, bool whole_grid, PushGround &g)
{
	Context &c = g_context;
	const ParameterBlock &pb = c.blocks[block];
	if (whole_grid && (c.device_count > 1 || pb.shard_z_count)) return set_error(BeamformerLibErrorKind_InvalidAccess);
	if (!rf_layout(pb, g.l)) return false;
	g.ps = commit_block(block);
	if (!g.ps) return set_error(BeamformerLibErrorKind_InvalidComputeStage);
	const Plan &plan = g.ps->plan;
	shard_planes(pb, plan, g.z_first, g.z_count);
	g.points[0] = plan.output_points[0]; g.points[1] = plan.output_points[1]; g.points[2] = g.z_count;
	return true;
}

/* A frame of the push's own grid, from RF frame rf_frame's DAS input */
static DasJob grid_job(const PushGround &g, const std::vector<DasDecision> *parts, uint32_t rf_frame, bool fused)
{
	DasJob j{};
	j.rf_frame = rf_frame; j.points = g.points; j.z_first = g.z_first;
	j.parts = parts; j.fused = fused; j.group = -1;
	return j;
}

/* A frame of a view's grid: its whole grid, whatever the block's */
static DasJob view_job(const BeamformerHipView &view, const std::vector<DasDecision> &parts, uint32_t rf_frame, bool fused)
{
	DasJob j{};
	j.rf_frame = rf_frame; j.points = view.output_points; j.tag = view.image_plane_tag;
	j.parts = parts.empty() ? nullptr : &parts; j.fused = fused; j.group = -1;
	return j;
}

/* A push of several frames with ONE upload and ONE event set, on one device.  The push_* function below describes the frames (Push: the
 * job list, the fused launch, the decode step); this function runs them:
 *   RF        one upload into one pinned slot -- over the copy engine into device staging when it is large, read in place over PCIe when
 *             small, by kOverlapBytes applied to the whole upload -- and ONE slot of the RF ring, frame k at k * rf_stride with 64 spare
 *             bytes behind every frame;
 *   stages    ingest, then every pre-DAS stage, ONE launch each for all RF frames: the stage kernels carry a frame dimension (grid z, or
 *             grid y beside the channels for the filters, which then take a burst in chunks of 65535 / channels frames) and address and
 *             bound every frame as a single frame is; several RF frames: frame k of a stage's output at k * stage_stride of burst_stage[],
 *             one: the single push's d.scratch[];
 *   DAS       the jobs of walk_plan;
 *   frames    contiguous in the frame ring, each rounded to 64 bytes (a run that would straddle the end starts again at 0), consecutive
 *             ids in job order;
 *   timings   one event set for the push, in the timing slot of its last frame; every frame's slot points there with share = frames.
 * Everything that can be refused is checked, and every buffer whose absence would fail the push is grown, BEFORE the ids are taken: a
 * refused push queues nothing.  (The tables some single-frame kernels keep -- staged_tables, hercules_table, hercules_pairs -- are grown
 * where a frame's launch asks for them, launch_das_part, each with a kernel to fall back on: growing one mid-push drains the device and
 * fails nothing.)  After that a failure leaves tombstones under all of its ids.  True: d.multi records the push, but for its route,
 * which the caller adds. */
static bool push_frames(uint32_t block, const PushGround &g, const void *data, bool data_on_device, Push &m)
{
	Context &c = g_context;
	Device  &d = *c.cur;
	const ParameterBlock &pb = c.blocks[block];
	PlanState *ps = g.ps;
	const Plan &plan = ps->plan;
	const RfLayout &l = g.l;
	hipStream_t s = d.stream;
	const uint32_t N = m.rf_frames, F = m.frames;

	uint64_t run_bytes = 0;
	if (!job_run_bytes(m.jobs, F, plan.iq_pipeline ? 8u : 4u, d.ring.size, run_bytes)) return set_error(BeamformerLibErrorKind_FrameSizeOverflow);

	/* device and pinned memory, grown before anything is queued */
	const uint64_t rf_stride = round_up(l.rf_size, 64) + 64;
	const uint64_t total     = (uint64_t)m.rf_frame_size * N;
	const uint32_t slot = (uint32_t)(d.rf_index % BeamformerMaxRawDataFramesInFlight);
	/* the route: decide_upload, as a push of several frames (the ingest kernel always runs) */
	const UploadDecision route = decide_upload(l, plan, m.rf_frame_size, N, true, data_on_device ? data : nullptr);
	const bool overlap = route.overlap;
	bool fits = d.rf[slot].ensure(rf_stride * N);
	m.stage = N > 1 ? d.burst_stage : d.scratch;
	m.stage_stride = N > 1 ? round_up(plan.intermediate_bytes, 64) + 64 : 0;
	if (m.stage_stride) {
		size_t pre_das_stages = 0;
		for (size_t i = 0; i < plan.stages.size(); i++) {
			const int kind = plan.stages[i].kind;
			if (kind == BeamformerShaderKind_DAS) break;
			pre_das_stages += kind != BeamformerShaderKind_CoherencyWeighting;
		}
		for (size_t k = 0; k < 2 && k < pre_das_stages; k++) fits = fits && m.stage[k].ensure(m.stage_stride * N);
	}
	if (overlap) fits = fits && d.raw_staging[slot].ensure(round_up(total, 64) + 64);
	if (m.decode_groups) fits = fits && d.readi_decoded.ensure(round_up(m.decoded_bytes, 64) + 64);
	if (m.decode_groups || (m.fused.kind != FusedLaunch::None && m.fused.kind != FusedLaunch::Burst)) {
		/* what stage_table goes through (one size for all users: a sweep's BEAMFORMER_HIP_MAX_BURST_FRAMES group ids are 4 KiB of it) */
		const size_t table_bytes = (sizeof(BfViewRow) + sizeof(uint32_t)) * BEAMFORMER_HIP_MAX_VIEWS + sizeof(uint32_t);
		fits = fits && d.views_table.ensure(table_bytes);
		if (fits && !d.views_pinned && !HIP_OK(hipHostMalloc(&d.views_pinned, table_bytes, hipHostMallocDefault))) { d.views_pinned = nullptr; fits = false; }
		if (fits && !d.views_copied && !HIP_OK(hipEventCreateWithFlags(&d.views_copied, hipEventDisableTiming))) { d.views_copied = nullptr; fits = false; }
	}
	if (!fits) { (void)hipGetLastError(); return set_error(BeamformerLibErrorKind_RFDataSizeOverflow); }
	UploadSlot &u = d.upload[slot];
	if (!claim_upload(u, total, !data_on_device)) return false;
	const uint32_t owner = (uint32_t)((c.push_sequence + F - 1) % kTimingSlots);     /* the push's events: its LAST frame's slot */
	TimingSlot &t = d.timing[owner];
	if (!ensure_events(t)) return false;
	if (c.count_pairs && !d.pair_counter.ensure(sizeof(unsigned long long) * (kTimingSlots + 2))) return set_error(BeamformerLibErrorKind_RFDataSizeOverflow);
	if (wants_counters(m.jobs, F) && !d.staged_violations.ensure(sizeof(uint32_t) * 4 * kTimingSlots)) return set_error(BeamformerLibErrorKind_RFDataSizeOverflow);

	/* ---- from here on the push owns ids first .. first + F - 1 ---- */
	d.rf_index++;
	const uint64_t first = c.push_sequence;
	c.push_sequence += F;
	d.frame_counter = first;
	d.multi.kind = PushRecord::None;
	Tombstones lockstep{c, first, F, 1, false};

	t.failed = false; t.sampled = true; t.events_slot = owner; t.share = F; t.count = 0; t.counted = false;
	d.have_sample = false;          /* the push's events cover F frames: a single frame that follows records its own */
	bool ok = HIP_OK(hipEventRecord(t.events[0], s));

	/* ---- upload and ingest: a multi-frame push always runs the ingest kernel.  One RF frame: strides 0, as in a single push ---- */
	const uint64_t in_step = route.in_step, rf_step = route.rf_step;
	const void *raw = data;
	if (!data_on_device) {
		raw = enqueue_upload(d, u, data, total, overlap ? d.raw_staging[slot].ptr : nullptr, total);
		if (!raw) return set_error(BeamformerLibErrorKind_InvalidAccess);
	}
	ok &= launch_ingest(ps, pb, l, raw, d.rf[slot].ptr, N, in_step, rf_step, s);
	if (route.zero_copy) ok &= pinned_read_by(u, s);
	segment(t, kStageIngest, s);
	if (!ok) return set_error(BeamformerLibErrorKind_InvalidAccess);
	note_push_time();
	d.last_rf = (char *)d.rf[slot].ptr + (N - 1) * rf_stride; d.last_rf_bytes = l.rf_size; d.last_rf_slot = slot; d.last_rf_sum_ready = false;

	/* ---- stages, one after the other over all RF frames.  What the first stage may read: each frame's RF itself (a later stage: what
	 * the plan's stages can have written of a stage buffer's frame, plan.intermediate_bytes) ---- */
	m.in = d.rf[slot].ptr; m.in_stride = rf_step; m.in_bound = (int64_t)l.rf_size;
	m.t = &t;
	const bool done = walk_plan(block, ps, m);
	finish_upload(u, overlap, s);
	if (!done) return false;

	share_timing_rows(d, first, F, owner);
	PushRecord &r = d.multi;
	r.kind = m.kind; r.first_id = first; r.count = F; r.events_slot = owner; r.decide_us = m.decide_us;
	r.rf_frames = N; r.mixed = 0;
	lockstep.complete = true;
	return true;
}

/* beamformer_hip_push_data_burst_with_compute: frame_count (two or more: one goes to the single push) RF frames of one parameter block
 * in one call, frame_count frames of the block's grid (its shard's planes).  The route: decide_burst on the block's own single-frame
 * decision.
 * beamformer_hip_push_data_readi_sweep_with_compute (groups given): a burst of a READI block whose frame k is beamformed with
 * readi_group = groups[k] (frame_count ids, every one below the block's readi_group_count: lib_api.cpp has checked both).  The route:
 * decide_burst as a sweep. */
bool push_burst(uint32_t block, const void *data, uint32_t frame_size, uint32_t frame_count, const uint32_t *groups, bool data_on_device)
{
	Context &c = g_context;
	Device  &d = *c.cur;
	const ParameterBlock &pb = c.blocks[block];
	const uint32_t N = frame_count;
	PushGround g;
	if (!begin_push(block, false, g)) return false;
	const Plan &plan = g.ps->plan;

	const std::vector<DasDecision> no_parts, *parts = frame_das_parts(g.ps, pb, g.z_first, g.z_count);
	BurstDecision route;
	decide_burst(pb, plan, g.ps->transmit_table, parts ? *parts : no_parts, g.z_first, g.z_count, c.das_path_mode, N, route, groups != nullptr);

	std::vector<DasJob> jobs(N);
	for (uint32_t k = 0; k < N; k++) {
		jobs[k] = grid_job(g, parts, k, route.burst_kernel);
		if (groups) jobs[k].group = (int32_t)groups[k];
	}
	Push m;
	m.kind = PushRecord::Burst; m.rf_frames = N; m.rf_frame_size = frame_size;
	m.jobs = jobs.data(); m.frames = N; m.das_ps = g.ps;
	if (route.burst_kernel) { m.fused.kind = groups ? FusedLaunch::ReadiSweep : FusedLaunch::Burst; m.fused.burst = &route; m.fused.groups = groups; }
	if (!push_frames(block, g, data, data_on_device, m)) return false;
	d.multi.burst = route;
	return true;
}

/* beamformer_hip_push_data_readi_image_with_compute: the sweep's RF frames and group ids (lib_api.cpp has checked the block, the list
 * and G x A), ONE frame: the derived block's single-frame DAS launch(es) on the DAS input decoded across the acquisitions. */
bool push_readi_image(uint32_t block, const void *data, uint32_t frame_size, uint32_t frame_count, const uint32_t *groups, bool data_on_device)
{
	Context &c = g_context;
	Device  &d = *c.cur;
	const ParameterBlock &pb = c.blocks[block];
	const uint32_t N = frame_count;
	PushGround g;
	if (!begin_push(block, false, g)) return false;
	ImagePlanState *image = commit_image_plan(block, g.ps);
	if (!image) return set_error(BeamformerLibErrorKind_RFDataSizeOverflow);
	const Plan &plan = g.ps->plan;

	const std::vector<DasDecision> no_parts, *parts = frame_das_parts(&image->ps, image->pb, g.z_first, g.z_count);
	ReadiImageDecision route;
	decide_readi_image(image->ps.plan, parts ? *parts : no_parts, pb.parameters.readi_group_count, N, route);

	DasJob one = grid_job(g, parts, 0, false);
	Push m;
	m.kind = PushRecord::Image; m.rf_frames = N; m.rf_frame_size = frame_size;
	m.jobs = &one; m.frames = 1; m.das_ps = &image->ps;
	m.decode_groups = groups;
	m.decoded_bytes = (uint64_t)plan.channels * image->ps.plan.acquisitions * plan.das_samples * (plan.iq_pipeline ? 8u : 4u);
	if (!push_frames(block, g, data, data_on_device, m)) return false;
	d.multi.image = route;
	return true;
}

/* The record of the newest multi-frame push, when the newest push IS that push, of `kind` and complete: waited for, with its stage
 * kinds and times (hipEvent pairs around each stage of the WHOLE push; total: first event to last).  Else null, InvalidAccess. */
static const PushRecord *newest_push(PushRecord::Kind kind, uint32_t &first_id, uint32_t &count, uint32_t &stage_count, uint32_t *stage_kind,
                                     float *stage_ms, float &total_ms)
{
	Context &c = g_context;
	Device &d = c.devices[0];
	const PushRecord &r = d.multi;
	if (!c.device_ready || r.kind != kind || d.frame_counter != r.first_id + r.count + r.mixed || !newest_record(d) ||
	    !HIP_OK(hipSetDevice(d.device)) || !HIP_OK(hipStreamSynchronize(d.stream))) {
		set_error(BeamformerLibErrorKind_InvalidAccess);
		return nullptr;
	}
	first_id = (uint32_t)r.first_id; count = r.count;
	const TimingSlot &t = d.timing[r.events_slot];
	stage_count = t.count;
	for (uint32_t i = 0; i < t.count; i++) {
		stage_kind[i] = t.kinds[i];
		float ms = 0;
		if (HIP_OK(hipEventElapsedTime(&ms, t.events[i], t.events[i + 1]))) stage_ms[i] = ms;
	}
	float total = 0;
	if (t.count && HIP_OK(hipEventElapsedTime(&total, t.events[0], t.events[t.count]))) total_ms = total;
	return &r;
}

/* A DAS path in the words of the C ABI: -2 the zero kernel, -1 none (no DAS stage runs: an empty part list), else the DasPath. */
static int abi_path(int path) { return path == DasPath_Zero ? -2 : path; }
static int abi_path(const std::vector<DasDecision> &parts) { return parts.empty() ? -1 : abi_path(main_part(parts).path); }

/* beamformer_hip_describe_burst, _describe_readi_sweep / _get_last_burst_info: a decision in the words of the C ABI */
void describe_burst_decision(const BurstDecision &route, BeamformerHipBurstDescription *out)
{
	std::memset(out, 0, sizeof(*out));
	out->burst_kernel = route.burst_kernel; out->single_path = abi_path(route.single_path);
	out->frames_per_thread = route.frames_per_thread; out->das_launches = route.das_launches;
	out->stage_launches = route.stage_launches; out->min_frames = route.min_frames;
	std::snprintf(out->reason, sizeof(out->reason), "%s", route.reason.c_str());
}

/* beamformer_hip_get_last_burst_info */
bool last_burst_info(BeamformerHipBurstInfo *out)
{
	std::memset(out, 0, sizeof(*out));
	const PushRecord *r = newest_push(PushRecord::Burst, out->first_frame_id, out->frame_count, out->stage_count, out->stage_kind, out->stage_ms, out->burst_ms);
	if (!r) return false;
	describe_burst_decision(r->burst, &out->route);
	return true;
}

/* beamformer_hip_describe_readi_image / _get_last_readi_image_info: a decision in the words of the C ABI */
void describe_readi_image_decision(const ReadiImageDecision &route, BeamformerHipReadiImageDescription *out)
{
	std::memset(out, 0, sizeof(*out));
	out->transmit_count = route.transmit_count;
	out->das_path = abi_path(route.path);
	out->das_launches = route.das_launches; out->stage_launches = route.stage_launches; out->decode_launches = route.decode_launches;
	std::snprintf(out->reason, sizeof(out->reason), "%s", route.reason.c_str());
}

/* beamformer_hip_get_last_readi_image_info */
bool last_readi_image_info(BeamformerHipReadiImageInfo *out)
{
	std::memset(out, 0, sizeof(*out));
	uint32_t count = 0;
	const PushRecord *r = newest_push(PushRecord::Image, out->frame_id, count, out->stage_count, out->stage_kind, out->stage_ms, out->image_ms);
	if (!r) return false;
	describe_readi_image_decision(r->image, &out->route);
	out->rf_frame_count = r->rf_frames;
	return true;
}

std::vector<ViewGrid> view_grids(const BeamformerHipView *views, uint32_t view_count)
{
	std::vector<ViewGrid> grids(view_count);
	for (uint32_t k = 0; k < view_count; k++) {
		std::memcpy(grids[k].transform, views[k].das_voxel_transform, sizeof(grids[k].transform));
		for (int i = 0; i < 3; i++) grids[k].points[i] = views[k].output_points[i];
	}
	return grids;
}

/* beamformer_hip_describe_views / _get_last_views_info: a decision in the words of the C ABI */
void describe_views_decision(const ViewsDecision &route, uint32_t view_count, BeamformerHipViewsDescription *out)
{
	std::memset(out, 0, sizeof(*out));
	out->kernel_views = route.kernel_views; out->das_launches = route.das_launches; out->min_tiles = kViewsMinTiles;
	for (uint32_t k = 0; k < view_count && k < BEAMFORMER_HIP_MAX_VIEWS; k++) out->path[k] = (int8_t)abi_path(route.parts[k]);
	std::snprintf(out->reason, sizeof(out->reason), "%s", route.reason.c_str());
}

/* beamformer_hip_push_data_views_with_compute: ONE RF frame beamformed on view_count grids (no output shard), view k's frame at its own
 * size.  The route: decide_views -- each view's own single-frame decision, and which of them the views kernel takes. */
bool push_views(uint32_t block, const void *data, uint32_t size, const BeamformerHipView *views, uint32_t view_count, bool data_on_device)
{
	Context &c = g_context;
	Device  &d = *c.cur;
	const uint32_t K = view_count;
	PushGround g;
	if (!begin_push(block, true, g)) return false;

	const auto decide_begin = std::chrono::steady_clock::now();
	ViewsDecision route;
	decide_views(c.blocks[block], g.ps->plan, g.ps->transmit_table, view_grids(views, K).data(), K, c.das_path_mode, route);
	const float decide_us = std::chrono::duration<float, std::micro>(std::chrono::steady_clock::now() - decide_begin).count();

	std::vector<DasJob> jobs(K);
	for (uint32_t k = 0; k < K; k++) jobs[k] = view_job(views[k], route.parts[k], 0, route.taken[k] != 0);
	Push m;
	m.kind = PushRecord::Views; m.rf_frame_size = size; m.decide_us = decide_us;
	m.jobs = jobs.data(); m.frames = K; m.das_ps = g.ps;
	if (route.kernel_views) { m.fused.kind = FusedLaunch::Views; m.fused.views = &route; }
	m.fails_on_flag = true;
	if (!push_frames(block, g, data, data_on_device, m)) return false;
	describe_views_decision(route, K, &d.multi.views);
	return true;
}

/* beamformer_hip_get_last_views_info */
bool last_views_info(BeamformerHipViewsInfo *out)
{
	std::memset(out, 0, sizeof(*out));
	const PushRecord *r = newest_push(PushRecord::Views, out->first_frame_id, out->view_count, out->stage_count, out->stage_kind, out->stage_ms, out->views_ms);
	if (!r) return false;
	out->route = r->views; out->decide_us = r->decide_us;
	return true;
}

/* beamformer_hip_describe_burst_views / _get_last_burst_views_info: a decision in the words of the C ABI */
void describe_burst_views_decision(const BurstViewsDecision &route, uint32_t view_count, BeamformerHipBurstViewsDescription *out)
{
	std::memset(out, 0, sizeof(*out));
	out->rung = route.rung; out->kernel_views = route.kernel_views; out->frame_kernel_views = route.frame_kernel_views;
	out->das_launches = route.das_launches; out->stage_launches = route.stage_launches;
	out->frames_per_thread = route.frames_per_thread; out->min_frames = route.min_frames;
	for (uint32_t k = 0; k < view_count && k < BEAMFORMER_HIP_MAX_VIEWS; k++) out->path[k] = (int8_t)abi_path(route.views.parts[k]);
	std::snprintf(out->reason, sizeof(out->reason), "%s", route.reason.c_str());
}

/* beamformer_hip_push_data_burst_views_with_compute: frame_count RF frames beamformed on view_count grids (no output shard),
 * frame_count x view_count frames view-major (frame v * N + k: view v, RF frame k), each at its view's size.  The route:
 * decide_burst_views -- ONE decide_das_parts per view, not per frame --, a ladder: its fused launch (das_burst_views.hip), or per RF
 * frame the views push's DAS step, or every frame its own launch(es). */
bool push_burst_views(uint32_t block, const void *data, uint32_t frame_size, uint32_t frame_count, const BeamformerHipView *views, uint32_t view_count,
                      bool data_on_device)
{
	Context &c = g_context;
	Device  &d = *c.cur;
	const uint32_t N = frame_count, K = view_count;
	PushGround g;
	if (!begin_push(block, true, g)) return false;

	const auto decide_begin = std::chrono::steady_clock::now();
	BurstViewsDecision route;
	decide_burst_views(c.blocks[block], g.ps->plan, g.ps->transmit_table, view_grids(views, K).data(), K, c.das_path_mode, N, route);
	const float decide_us = std::chrono::duration<float, std::micro>(std::chrono::steady_clock::now() - decide_begin).count();

	/* (`fused` also names the jobs the views kernel covers per RF frame, rung 2) */
	std::vector<DasJob> jobs((size_t)N * K);
	for (uint32_t v = 0; v < K; v++)
		for (uint32_t k = 0; k < N; k++) jobs[(size_t)v * N + k] = view_job(views[v], route.views.parts[v], k, route.views.taken[v] != 0);
	Push m;
	m.kind = PushRecord::BurstViews; m.rf_frames = N; m.rf_frame_size = frame_size; m.decide_us = decide_us;
	m.jobs = jobs.data(); m.frames = N * K; m.das_ps = g.ps;
	if (route.views.kernel_views) { m.fused.kind = route.rung == 1 ? FusedLaunch::BurstViews : FusedLaunch::ViewsPerRfFrame; m.fused.views = &route.views; }
	m.fails_on_flag = true;
	if (!push_frames(block, g, data, data_on_device, m)) return false;
	describe_burst_views_decision(route, K, &d.multi.burst_views);
	return true;
}

/* beamformer_hip_get_last_burst_views_info */
bool last_burst_views_info(BeamformerHipBurstViewsInfo *out)
{
	std::memset(out, 0, sizeof(*out));
	uint32_t frames = 0;
	const PushRecord *r = newest_push(PushRecord::BurstViews, out->first_frame_id, frames, out->stage_count, out->stage_kind, out->stage_ms, out->push_ms);
	if (!r) return false;
	out->route = r->burst_views; out->decide_us = r->decide_us;
	out->frame_count = r->rf_frames; out->view_count = r->rf_frames ? frames / r->rf_frames : 0;
	return true;
}

/* beamformer_hip_describe_variants / _get_last_variants_info: a decision in the words of the C ABI */
void describe_variants_decision(const VariantsDecision &route, uint32_t variant_count, BeamformerHipVariantsDescription *out)
{
	std::memset(out, 0, sizeof(*out));
	out->kernel_variants = route.kernel_variants; out->fused_launches = route.kernel_variants ? 1u : 0u;
	out->das_launches = route.das_launches; out->kernel_tiles = route.kernel_tiles; out->min_tiles = kVariantsMinTiles;
	out->min_variants = kVariantsMinVariants;
	for (uint32_t k = 0; k < variant_count && k < BEAMFORMER_HIP_MAX_VARIANTS; k++) {
		out->taken[k] = route.taken[k];
		out->path[k] = (int8_t)abi_path(route.parts[k]);
	}
	std::snprintf(out->reason, sizeof(out->reason), "%s", route.reason.c_str());
}

static bool same_variant(const DasVariant &a, const DasVariant &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

/* beamformer_hip_push_data_variants_with_compute: ONE RF frame beamformed on the block's grid (no output shard) under variant_count
 * triples of speed of sound, time offset and f-number: das_variants.hip for the variants decide_variants gives it, every other variant
 * its own launch(es) under its derived decision.  The block is read, never written: no dirty bit, no replan.  The route:
 * decide_variants -- each variant's own single-frame decision under its derived block, kept in the block's derived plan states
 * (context.h: VariantPlanState) and reused by later pushes of the same triple, and which of them the variants kernel takes. */
bool push_variants(uint32_t block, const void *data, uint32_t size, const DasVariant *variants, uint32_t variant_count, bool data_on_device)
{
	Context &c = g_context;
	Device  &d = *c.cur;
	const ParameterBlock &pb = c.blocks[block];
	const uint32_t K = variant_count;
	PushGround g;
	if (!begin_push(block, true, g)) return false;
	PlanState *ps = g.ps;

	const auto decide_begin = std::chrono::steady_clock::now();
	std::list<VariantPlanState> &kept = d.variant_plans[block];
	auto current = [&](const VariantPlanState &vp, const DasVariant &v) {
		return same_variant(vp.variant, v) && vp.source_generation == ps->generation && vp.mode == c.das_path_mode && vp.hooks_version == hooks().version;
	};
	if (kept.size() + K > kMaxVariantPlans) kept.clear();
	std::vector<const std::vector<DasDecision> *> known(K, nullptr);
	for (uint32_t k = 0; k < K; k++)
		for (const VariantPlanState &vp : kept)
			if (current(vp, variants[k])) { known[k] = &vp.parts; break; }
	VariantsDecision route;
	decide_variants(pb, ps->plan, ps->transmit_table, variants, K, c.das_path_mode, route, known.data());
	for (uint32_t k = 0; k < K; k++) {
		if (known[k] || route.parts[k].empty()) continue;
		bool listed = false;                         /* (the same triple twice in one push) */
		for (const VariantPlanState &vp : kept) listed |= current(vp, variants[k]);
		if (!listed) kept.push_back(VariantPlanState{variants[k], route.parts[k], ps->generation, hooks().version, c.das_path_mode});
	}
	const float decide_us = std::chrono::duration<float, std::micro>(std::chrono::steady_clock::now() - decide_begin).count();

	std::vector<DasJob> jobs(K);
	for (uint32_t k = 0; k < K; k++) jobs[k] = grid_job(g, route.parts[k].empty() ? nullptr : &route.parts[k], 0, route.taken[k] != 0);
	Push m;
	m.kind = PushRecord::Variants; m.rf_frame_size = size; m.decide_us = decide_us;
	m.jobs = jobs.data(); m.frames = K; m.das_ps = ps;
	if (route.kernel_variants) { m.fused.kind = FusedLaunch::Variants; m.fused.variants = &route; }
	m.fails_on_flag = true;
	if (!push_frames(block, g, data, data_on_device, m)) return false;
	describe_variants_decision(route, K, &d.multi.variants);
	return true;
}

/* beamformer_hip_get_last_variants_info */
bool last_variants_info(BeamformerHipVariantsInfo *out)
{
	std::memset(out, 0, sizeof(*out));
	const PushRecord *r = newest_push(PushRecord::Variants, out->first_frame_id, out->variant_count, out->stage_count, out->stage_kind, out->stage_ms, out->variants_ms);
	if (!r) return false;
	out->route = r->variants; out->decide_us = r->decide_us;
	return true;
}

/* the reference waits on futex locks with a timeout (lib .c:192-198, :679);
 * (uint32_t)-1 blocks forever */
bool wait_for_frames(int32_t timeout_ms)
{
	Context &c = g_context;
	if (!c.device_ready) return true;
	auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(timeout_ms < 0 ? 0 : timeout_ms);
	bool ok = true;
	for (uint32_t i = 0; i < c.device_count && ok; i++) {
		Device &d = c.devices[i];
		if (!HIP_OK(hipSetDevice(d.device))) { ok = set_error(BeamformerLibErrorKind_InvalidAccess); break; }
		if (timeout_ms < 0) { ok = HIP_OK(hipStreamSynchronize(d.stream)) || set_error(BeamformerLibErrorKind_InvalidAccess); continue; }
		for (;;) {
			hipError_t e = hipStreamQuery(d.stream);
			if (e == hipSuccess) break;
			if (e != hipErrorNotReady) { ok = set_error(BeamformerLibErrorKind_InvalidAccess); break; }
			if (std::chrono::steady_clock::now() >= deadline) { ok = set_error(BeamformerLibErrorKind_SyncVariable); break; }
			std::this_thread::sleep_for(std::chrono::microseconds(50));
		}
	}
	(void)hipSetDevice(c.devices[0].device);
	c.cur = &c.devices[0];
	return ok;
}

/* The record of device d's newest frame -- or null when the newest push did not complete (its slot holds a tombstone) or the slot still
 * holds an older frame's record: every reader of "the last frame" goes through here and fails instead of serving a stale record. */
const FrameRecord *newest_record(const Device &d)
{
	if (d.frame_counter == 0 || d.frames.empty()) return nullptr;
	const uint64_t id = d.frame_counter - 1;
	const FrameRecord &f = d.frames[id % d.frames.size()];
	return (f.id == (uint32_t)id && !f.failed) ? &f : nullptr;
}

/* BeamformerExportKind_BeamformedData (beamformer_core.c:1474-1494) */
bool export_last_frames(void *out, uint64_t out_size, uint32_t count, int32_t timeout_ms)
{
	Context &c = g_context;
	Device  &d = c.devices[0];
	if (!wait_for_frames(timeout_ms)) return false;
	if (d.frame_counter == 0) return set_error(BeamformerLibErrorKind_InvalidAccess);
	uint64_t req = count < 1 ? 1 : count;
	if (req > d.frame_counter) req = d.frame_counter;
	if (req > d.frames.size()) req = d.frames.size();
	uint64_t index = d.frame_counter - req, exported = 0;
	bool ok = true;
	if (c.device_count == 1) {
		for (uint64_t n = 0; n < req; n++, index++) {
			const FrameRecord &f = d.frames[index % d.frames.size()];
			const bool present = f.id == (uint32_t)index && !f.failed && f.bytes;
			/* older frames that are gone (storage reused, a push that failed) are skipped; the NEWEST one missing is an error, not a
			 * success that leaves the caller's buffer unwritten */
			if (!present) { if (n + 1 == req) ok = false; continue; }
			if (exported + f.bytes <= out_size) {
				ok &= HIP_OK(hipMemcpyAsync((char *)out + exported, (const char *)d.ring.ptr + f.offset, f.bytes,
				                            hipMemcpyDeviceToHost, d.stream));
				exported += f.bytes;
			}
		}
		ok &= HIP_OK(hipStreamSynchronize(d.stream));
		return ok || set_error(BeamformerLibErrorKind_InvalidAccess);
	}
	/* several devices: every frame id exists on each of them as one z-slab (devices run in lockstep);
	 * the caller sees whole frames, slabs stitched in z order, each frame rounded to 64 bytes exactly
	 * as a single device would have exported it */
	for (uint64_t n = 0; n < req; n++, index++) {
		uint64_t voxels = 0, elem = 0; bool valid = true;
		for (uint32_t i = 0; i < c.device_count; i++) {
			const FrameRecord &f = c.devices[i].frames[index % c.devices[i].frames.size()];
			if (f.id != (uint32_t)index || f.failed) { valid = false; break; }
			uint64_t v = (uint64_t)f.points[0] * f.points[1] * f.points[2];
			if (v && !f.bytes) { valid = false; break; }              /* storage reused by a newer frame */
			voxels += v; if (v) elem = (uint64_t)bf_kind_byte_size[f.data_kind];
		}
		uint64_t whole = round_up(voxels * elem, 64);
		if (!valid || !whole) {
			/* a device of the set holds no complete slab of this frame (a push that failed half way, storage reused): older frames
			 * are skipped as in the one-device export; the NEWEST frame missing is an error, not an unwritten buffer */
			if (n + 1 == req) { ok = false; break; }
			continue;
		}
		if (exported + whole > out_size) continue;
		uint64_t at = exported;
		for (uint32_t i = 0; i < c.device_count; i++) {
			Device &p = c.devices[i];
			const FrameRecord &f = p.frames[index % p.frames.size()];
			uint64_t bytes = (uint64_t)f.points[0] * f.points[1] * f.points[2] * elem;
			if (!bytes) continue;
			ok &= HIP_OK(hipSetDevice(p.device));
			ok &= HIP_OK(hipMemcpyAsync((char *)out + at, (const char *)p.ring.ptr + f.offset, bytes, hipMemcpyDeviceToHost, p.stream));
			at += bytes;
		}
		if (at < exported + whole) std::memset((char *)out + at, 0, exported + whole - at);   /* the rounding tail */
		exported += whole;
	}
	for (uint32_t i = 0; i < c.device_count; i++) {
		ok &= HIP_OK(hipSetDevice(c.devices[i].device));
		ok &= HIP_OK(hipStreamSynchronize(c.devices[i].stream));
	}
	(void)hipSetDevice(d.device);
	return ok || set_error(BeamformerLibErrorKind_InvalidAccess);
}

static bool timings_of(Device &d, BeamformerHipFrameTimings *out)
{
	std::memset(out, 0, sizeof(*out));
	if (d.frame_counter == 0) return set_error(BeamformerLibErrorKind_InvalidAccess);
	if (!HIP_OK(hipSetDevice(d.device)) || !HIP_OK(hipStreamSynchronize(d.stream))) return set_error(BeamformerLibErrorKind_InvalidAccess);
	TimingSlot &t = d.timing[(d.frame_counter - 1) % kTimingSlots];
	if (t.failed) return set_error(BeamformerLibErrorKind_InvalidAccess);          /* the newest push did not complete: no timings of an older frame in its place */
	TimingSlot &e = d.timing[t.events_slot];       /* t itself, or the newest sampled frame of the same plan */
	out->stage_count = t.count;
	for (uint32_t i = 0; i < t.count; i++) {
		out->stage_kind[i] = t.kinds[i];
		float ms = 0;
		if (HIP_OK(hipEventElapsedTime(&ms, e.events[i], e.events[i + 1]))) out->stage_ms[i] = ms / (float)t.share;
	}
	float total = 0;
	if (t.count && HIP_OK(hipEventElapsedTime(&total, e.events[0], e.events[t.count]))) out->frame_ms = total / (float)t.share;
	out->das_voxels = t.das_voxels; out->das_taps = t.das_taps;
	out->das_sample_bytes = t.das_sample_bytes; out->das_path = t.das_path;
	out->das_row_end_planes = t.das_row_end_planes;
	if (t.violations_slot != ~0ull && d.staged_violations.ptr) {
		uint32_t n[4] = {0, 0, 0, 0};
		(void)hipMemcpy(n, (uint32_t *)d.staged_violations.ptr + 4 * t.violations_slot, sizeof(n), hipMemcpyDeviceToHost);
		out->staged_window_violations = n[0];
		out->tile_staged_chunks = n[1]; out->tile_gather_chunks = n[2];
	}
	if (t.counted && d.pair_counter.ptr) {
		unsigned long long n = 0;
		(void)hipMemcpy(&n, (unsigned long long *)d.pair_counter.ptr + ((d.frame_counter - 1) % kTimingSlots),
		                sizeof(n), hipMemcpyDeviceToHost);
		out->das_pairs = n;
	}
	return true;
}

/* the newest frame as one device saw it (its slab, its events) */
bool device_frame_timings(uint32_t device_index, BeamformerHipFrameTimings *out)
{
	Context &c = g_context;
	std::memset(out, 0, sizeof(*out));
	if (!c.device_ready || device_index >= c.device_count) return set_error(BeamformerLibErrorKind_InvalidAccess);
	bool ok = timings_of(c.devices[device_index], out);
	(void)hipSetDevice(c.devices[0].device);
	return ok;
}

bool device_info(uint32_t device_index, BeamformerHipDeviceInfo *out)
{
	Context &c = g_context;
	std::memset(out, 0, sizeof(*out));
	if (!c.device_ready || device_index >= c.device_count) return set_error(BeamformerLibErrorKind_InvalidAccess);
	Device &d = c.devices[device_index];
	out->ordinal = d.device; out->peer_access = d.peer_access;
	out->slab_first = d.slab_first; out->slab_count = d.slab_count;
	bool ok = HIP_OK(hipSetDevice(d.device)) && HIP_OK(hipStreamSynchronize(d.stream));
	if (ok && d.frame_counter) {
		BeamformerHipFrameTimings t;
		if (timings_of(d, &t)) {
			out->frame_ms = t.frame_ms;
			for (uint32_t i = 0; i < t.stage_count; i++) if (t.stage_kind[i] == (uint32_t)BeamformerShaderKind_DAS) out->das_ms = t.stage_ms[i];
		}
		if (device_index != 0 && d.peer_copy_end[d.last_rf_slot]) {
			float ms = 0;
			if (HIP_OK(hipStreamSynchronize(d.peer_stream)) && HIP_OK(hipEventElapsedTime(&ms, d.peer_copy_begin[d.last_rf_slot], d.peer_copy_end[d.last_rf_slot]))) out->peer_copy_ms = ms;
			(void)hipGetLastError();
		}
		if (d.last_rf && d.last_rf_bytes) {
			ok = d.pair_counter.ensure(sizeof(unsigned long long) * (kTimingSlots + 2));
			unsigned long long *sum = ok ? (unsigned long long *)d.pair_counter.ptr + kTimingSlots : nullptr;
			unsigned long long host = 0;
			ok = ok && HIP_OK(bf_launch_rf_checksum(d.last_rf, d.last_rf_bytes, sum, d.stream)) &&
			     HIP_OK(hipMemcpyAsync(&host, sum, sizeof(host), hipMemcpyDeviceToHost, d.stream)) && HIP_OK(hipStreamSynchronize(d.stream));
			out->rf_checksum = host; out->rf_bytes = d.last_rf_bytes;
		} else if (d.last_rf_sum_ready && d.pair_counter.ptr) {
			/* a borrowed device buffer: summed inside the push (the caller may have freed it since) */
			unsigned long long host = 0;
			ok = HIP_OK(hipMemcpyAsync(&host, (unsigned long long *)d.pair_counter.ptr + kTimingSlots + 1, sizeof(host), hipMemcpyDeviceToHost, d.stream)) &&
			     HIP_OK(hipStreamSynchronize(d.stream));
			out->rf_checksum = host; out->rf_bytes = d.last_rf_bytes;
		}
	}
	(void)hipSetDevice(c.devices[0].device);
	return ok || set_error(BeamformerLibErrorKind_InvalidAccess);
}

/* the newest frame: stage times of the ingest device; with several devices the voxel and pair counts
 * are those of the whole frame and the frame time is the slowest device's */
bool last_frame_timings(BeamformerHipFrameTimings *out)
{
	Context &c = g_context;
	std::memset(out, 0, sizeof(*out));
	if (!c.device_ready) return set_error(BeamformerLibErrorKind_InvalidAccess);
	if (!timings_of(c.devices[0], out)) return false;
	for (uint32_t i = 1; i < c.device_count; i++) {
		BeamformerHipFrameTimings peer;
		if (!timings_of(c.devices[i], &peer)) { (void)hipSetDevice(c.devices[0].device); return false; }
		out->das_voxels += peer.das_voxels; out->das_pairs += peer.das_pairs;
		out->staged_window_violations += peer.staged_window_violations;
		out->tile_staged_chunks += peer.tile_staged_chunks; out->tile_gather_chunks += peer.tile_gather_chunks;
		out->das_row_end_planes += peer.das_row_end_planes;
		if (peer.frame_ms > out->frame_ms) out->frame_ms = peer.frame_ms;
	}
	(void)hipSetDevice(c.devices[0].device);
	return true;
}

/* BeamformerComputeStatsTable (beamformer_compute_stats.c:3-10) as coalesce_timing_table
 * (beamformer_core.c:1683-1747) fills it: seconds per planned stage for the last 32 frames; with
 * several devices each entry is the slowest device's (they run side by side) */
bool fill_stats_table(BeamformerComputeStatsTable *out)
{
	Context &c = g_context;
	std::memset(out, 0, sizeof(*out));
	if (!c.device_ready || c.devices[0].frame_counter == 0) return true;
	for (uint32_t dev = 0; dev < c.device_count; dev++) {
		Device &d = c.devices[dev];
		if (!HIP_OK(hipSetDevice(d.device)) || !HIP_OK(hipStreamSynchronize(d.stream))) {
			(void)hipSetDevice(c.devices[0].device);
			return set_error(BeamformerLibErrorKind_InvalidAccess);
		}
		uint64_t frames = d.frame_counter < kTimingSlots ? d.frame_counter : kTimingSlots;
		for (uint64_t n = 0; n < frames; n++) {
			uint64_t id = d.frame_counter - frames + n;
			TimingSlot &t = d.timing[id % kTimingSlots];
			if (t.failed) continue;                    /* a push that did not complete: its row stays zero */
			TimingSlot &e = d.timing[t.events_slot];
			uint32_t col = 0;
			for (uint32_t i = 0; i < t.count; i++) {
				if (t.kinds[i] == kStageIngest || t.kinds[i] == kStagePairCount) continue;
				if (col >= BeamformerMaxComputeShaderStages) break;
				float ms = 0;
				(void)hipEventElapsedTime(&ms, e.events[i], e.events[i + 1]);
				ms /= (float)t.share;                  /* a frame of a burst: its share of the burst's stage time */
				float &cell = out->times[id % 32][col];
				if (ms * 1e-3f > cell) cell = ms * 1e-3f;
				if (dev == 0 && n == frames - 1) out->shader_ids[col] = t.kinds[i];
				col++;
			}
			if (dev == 0 && n == frames - 1) out->shader_count = col;
		}
	}
	(void)hipSetDevice(c.devices[0].device);
	for (size_t i = 0; i < c.rf_time_deltas.size() && i < 32; i++) out->rf_time_deltas[i] = c.rf_time_deltas[i];
	return true;
}

/* byte offset of device `dev`'s slab inside the stitched newest frame, and the frame's total bytes */
static bool newest_layout(Context &c, uint64_t offsets[kMaxDevices], uint64_t per_voxel, uint64_t &total)
{
	total = 0;
	for (uint32_t i = 0; i < c.device_count; i++) {
		Device &p = c.devices[i];
		const FrameRecord *fp = newest_record(p);
		if (!fp) return false;
		const FrameRecord &f = *fp;
		offsets[i] = total;
		total += (uint64_t)f.points[0] * f.points[1] * f.points[2] * per_voxel;
	}
	return true;
}

/* beamformer_hip_copy_das_input_frame: what the DAS stage read for RF frame `frame` of the newest push, [channel][transmit][sample]; one
 * device only */
bool copy_das_input_frame(uint32_t frame, void *out, uint64_t out_size)
{
	Context &c = g_context;
	if (!c.device_ready || c.device_count != 1) return set_error(BeamformerLibErrorKind_InvalidAccess);
	Device &d = c.devices[0];
	if (!newest_record(d) || !d.das_input || frame >= d.das_input_frames || out_size != d.das_input_bytes) return set_error(BeamformerLibErrorKind_InvalidAccess);
	/* a parameter push since that push may have regrown (reallocated) the buffer: then there is nothing to copy */
	const uint64_t offset = (uint64_t)frame * d.das_input_stride, end = offset + out_size;
	bool live = false;
	for (const DeviceBuffer &b : d.scratch)     live |= b.ptr == d.das_input && b.size >= end;
	for (const DeviceBuffer &b : d.burst_stage) live |= b.ptr == d.das_input && b.size >= end;
	for (const DeviceBuffer &b : d.rf)          live |= b.ptr == d.das_input && b.size >= end;      /* (a plan with no pre-DAS stage) */
	if (!live) return set_error(BeamformerLibErrorKind_InvalidAccess);
	bool ok = HIP_OK(hipSetDevice(d.device));
	ok = ok && HIP_OK(hipMemcpyAsync(out, (const char *)d.das_input + offset, out_size, hipMemcpyDeviceToHost, d.stream));
	ok = ok && HIP_OK(hipStreamSynchronize(d.stream));
	return ok || set_error(BeamformerLibErrorKind_InvalidAccess);
}

/* beamformer_hip_copy_das_input: the newest frame's -- a single push's, a views push's one input, a burst's last frame */
bool copy_das_input(void *out, uint64_t out_size)
{
	Context &c = g_context;
	Device &d = c.devices[0];
	if (c.device_ready && c.device_count == 1 && d.das_decoded_bytes) {
		/* a READI image push: what its DAS stage read is the buffer decoded across the acquisitions, [channel][G x A][sample] */
		if (!newest_record(d) || !d.das_input || out_size != d.das_decoded_bytes || d.readi_decoded.size < out_size) return set_error(BeamformerLibErrorKind_InvalidAccess);
		bool ok = HIP_OK(hipSetDevice(d.device));
		ok = ok && HIP_OK(hipMemcpyAsync(out, d.readi_decoded.ptr, out_size, hipMemcpyDeviceToHost, d.stream));
		ok = ok && HIP_OK(hipStreamSynchronize(d.stream));
		return ok || set_error(BeamformerLibErrorKind_InvalidAccess);
	}
	const uint32_t frames = c.devices[0].das_input_frames;
	return copy_das_input_frame(frames ? frames - 1 : 0, out, out_size);
}

bool frame_min_max(float out[2])
{
	Context &c = g_context;
	if (!c.device_ready || c.devices[0].frame_counter == 0) return set_error(BeamformerLibErrorKind_InvalidAccess);
	bool ok = true, any = false;
	float lo = 0.f, hi = 0.f;
	for (uint32_t i = 0; i < c.device_count && ok; i++) {
		Device &d = c.devices[i];
		const FrameRecord *fp = newest_record(d);
		if (!fp) { ok = false; break; }
		const FrameRecord &f = *fp;
		uint64_t voxels = (uint64_t)f.points[0] * f.points[1] * f.points[2];
		if (!voxels) continue;
		ok &= HIP_OK(hipSetDevice(d.device));
		if (!ok || !d.minmax_scratch.ensure(sizeof(float) * (2 * 1024 + 2))) { ok = false; break; }
		float *scratch = (float *)d.minmax_scratch.ptr;
		float part[2];
		ok &= HIP_OK(bf_launch_min_max((const char *)d.ring.ptr + f.offset, voxels,
		                               f.data_kind == BeamformerDataKind_Float32Complex, scratch + 2, scratch, d.stream));
		ok &= HIP_OK(hipMemcpyAsync(part, scratch, 2 * sizeof(float), hipMemcpyDeviceToHost, d.stream));
		ok &= HIP_OK(hipStreamSynchronize(d.stream));
		/* the two-float combine across slabs; NaN voxels propagate as in the one-device reduction */
		if (!any) { lo = part[0]; hi = part[1]; any = true; }
		else {
			lo = (part[0] < lo || part[0] != part[0]) ? part[0] : lo;
			hi = (part[1] > hi || part[1] != part[1]) ? part[1] : hi;
		}
	}
	(void)hipSetDevice(c.devices[0].device);
	out[0] = lo; out[1] = hi;
	return (ok && any) || set_error(BeamformerLibErrorKind_InvalidAccess);
}

/* Rolling average of the `count` newest frames as the reference's Sum stage specifies it
 * (beamformer_core.c:1417-1448 + shaders/sum.glsl): cleared output, then one
 * out += (1/count) * frame pass per frame, oldest first.  The reference's planner drops
 * Sum from every pipeline (beamformer_core.c:632-637), so this is reachable only through
 * the extension and never changes what get_last_frames returns.  With several devices each
 * averages its own slab and the slabs are stitched in the caller's buffer. */
bool sum_last_frames(uint32_t count, void *out, uint64_t out_size)
{
	Context &c = g_context;
	if (!c.device_ready || c.devices[0].frame_counter == 0 || count == 0) return set_error(BeamformerLibErrorKind_InvalidAccess);
	uint64_t offsets[kMaxDevices], total = 0;
	{
		const FrameRecord *f0 = newest_record(c.devices[0]);
		if (!f0 || !newest_layout(c, offsets, (uint64_t)bf_kind_byte_size[f0->data_kind], total)) return set_error(BeamformerLibErrorKind_InvalidAccess);
	}
	if (out_size < round_up(total, 64)) return set_error(BeamformerLibErrorKind_ExportSpaceOverflow);
	bool ok = true;
	for (uint32_t i = 0; i < c.device_count && ok; i++) {
		Device &d = c.devices[i];
		if (count > d.frame_counter || count > d.frames.size()) return set_error(BeamformerLibErrorKind_InvalidAccess);
		const FrameRecord &newest = *newest_record(d);          /* (present: newest_layout checked every device) */
		uint64_t slab_bytes = (uint64_t)newest.points[0] * newest.points[1] * newest.points[2] * (uint64_t)bf_kind_byte_size[newest.data_kind];
		if (!slab_bytes) continue;
		for (uint64_t id = d.frame_counter - count; id < d.frame_counter; id++) {
			const FrameRecord &f = d.frames[id % d.frames.size()];
			if (f.id != (uint32_t)id || f.failed || !f.bytes || f.bytes != newest.bytes || f.data_kind != newest.data_kind ||
			    f.points[0] != newest.points[0] || f.points[1] != newest.points[1] || f.points[2] != newest.points[2])
				return set_error(BeamformerLibErrorKind_DataSizeMismatch);
		}
		ok &= HIP_OK(hipSetDevice(d.device));
		if (!ok || !d.sum_scratch.ensure(newest.bytes)) { ok = false; break; }
		ok &= HIP_OK(hipMemsetAsync(d.sum_scratch.ptr, 0, newest.bytes, d.stream));
		float prescale = 1.0f / (float)count;
		for (uint64_t id = d.frame_counter - count; ok && id < d.frame_counter; id++) {
			const FrameRecord &f = d.frames[id % d.frames.size()];
			ok &= HIP_OK(bf_launch_sum(d.sum_scratch.ptr, (const char *)d.ring.ptr + f.offset, prescale, f.bytes, d.stream));
		}
		/* one device: the whole 64-byte-rounded frame, as before; several: the slab's own bytes */
		uint64_t copy = c.device_count == 1 ? newest.bytes : slab_bytes;
		ok &= HIP_OK(hipMemcpyAsync((char *)out + offsets[i], d.sum_scratch.ptr, copy, hipMemcpyDeviceToHost, d.stream));
	}
	for (uint32_t i = 0; i < c.device_count; i++) {
		ok &= HIP_OK(hipSetDevice(c.devices[i].device));
		ok &= HIP_OK(hipStreamSynchronize(c.devices[i].stream));
	}
	(void)hipSetDevice(c.devices[0].device);
	return ok || set_error(BeamformerLibErrorKind_InvalidAccess);
}

/* Display intensities of the newest frame (render_3d.frag.glsl:50-73), one float per voxel. */
bool display_last_frame(float threshold_db, float gamma, float db_cutoff, float *out, uint64_t out_floats)
{
	Context &c = g_context;
	if (!c.device_ready || c.devices[0].frame_counter == 0) return set_error(BeamformerLibErrorKind_InvalidAccess);
	uint64_t offsets[kMaxDevices], total = 0;
	if (!newest_layout(c, offsets, 1, total)) return set_error(BeamformerLibErrorKind_InvalidAccess);
	if (out_floats < total) return set_error(BeamformerLibErrorKind_ExportSpaceOverflow);
	bool ok = true;
	for (uint32_t i = 0; i < c.device_count && ok; i++) {
		Device &d = c.devices[i];
		const FrameRecord &f = *newest_record(d);               /* (present: newest_layout checked every device) */
		uint64_t voxels = (uint64_t)f.points[0] * f.points[1] * f.points[2];
		if (!voxels) continue;
		ok &= HIP_OK(hipSetDevice(d.device));
		if (!ok || !d.sum_scratch.ensure(voxels * sizeof(float))) { ok = false; break; }
		ok &= HIP_OK(bf_launch_display((const char *)d.ring.ptr + f.offset, voxels, f.data_kind == BeamformerDataKind_Float32Complex,
		                               threshold_db, gamma, db_cutoff, (float *)d.sum_scratch.ptr, d.stream));
		ok &= HIP_OK(hipMemcpyAsync(out + offsets[i], d.sum_scratch.ptr, voxels * sizeof(float), hipMemcpyDeviceToHost, d.stream));
	}
	for (uint32_t i = 0; i < c.device_count; i++) {
		ok &= HIP_OK(hipSetDevice(c.devices[i].device));
		ok &= HIP_OK(hipStreamSynchronize(c.devices[i].stream));
	}
	(void)hipSetDevice(c.devices[0].device);
	return ok || set_error(BeamformerLibErrorKind_InvalidAccess);
}

/* The ring side of a run that frame_ops.cpp queues behind the newest frames (queue_frames_of_newest): `count` frames of `points`
 * voxels.  Where the ring's placement rule (place_frames) will put it; false: it does not fit the ring. */
bool queued_run_landing(const Device &d, const uint32_t points[3], uint32_t count, bool cplx, uint64_t &run_first, uint64_t &run_bytes)
{
	if (!run_bytes_of([points](uint32_t) { return FrameShape{points, 0}; }, count, cplx ? 8u : 4u, d.ring.size, run_bytes)) return false;
	run_first = d.ring_next_offset > d.ring.size - run_bytes ? 0 : d.ring_next_offset;
	return true;
}

/* ... and the run itself: ids first .. first + M - 1, taken from the counters a push advances, its frames placed, their timing slots
 * reset; then enqueue(first, the first frame's record), whose result is the call's: false leaves tombstones under the ids, as a push does */
bool claim_queued_run(Device &d, const uint32_t points[3], uint32_t tag, uint32_t M, bool cplx, uint32_t block,
                      const std::function<bool(uint64_t first, const FrameRecord &frame0)> &enqueue)
{
	const uint64_t first = g_context.push_sequence;
	g_context.push_sequence += M;
	d.frame_counter = first;
	Tombstones lockstep{g_context, first, M, 1, false};
	/* the newest push stays the newest push behind the run -- unless the run takes the timing slot that holds its events */
	PushRecord &push = d.multi;
	if (push.kind != PushRecord::None && first == push.first_id + push.count + push.mixed) {
		bool slot_taken = M >= kTimingSlots;
		for (uint32_t j = 0; j < M && !slot_taken; j++) slot_taken = (first + j) % kTimingSlots == push.events_slot;
		if (slot_taken) push.kind = PushRecord::None; else push.mixed += M;
	}
	uint64_t run_bytes = 0;
	FrameRecord *frame0 = place_frames([points, tag](uint32_t) { return FrameShape{points, tag}; }, M, cplx, block, run_bytes);
	if (!frame0) return set_error(BeamformerLibErrorKind_FrameSizeOverflow);      /* (queued_run_landing has checked it: not reached) */
	for (uint32_t j = 0; j < M; j++) {
		TimingSlot &t = d.timing[(first + j) % kTimingSlots];
		t.count = 0; t.counted = false; t.sampled = false; t.events_slot = (uint32_t)((first + j) % kTimingSlots); t.share = 1;
		t.das_voxels = 0; t.das_taps = t.das_sample_bytes = t.das_path = 0; t.das_row_end_planes = 0;
		t.violations_slot = ~0ull; t.frame_id = first + j; t.failed = false;
	}
	d.have_sample = false;              /* the slots of older sampled frames may be gone: a single frame that follows records its own events */
	return lockstep.complete = enqueue(first, *frame0);
}

/* The record of the frame with this id, while the frame is still there: its record not yet overwritten (the newest frames.size() ids),
 * no tombstone, its ring storage not reused by a newer frame (next_frames clears `bytes` then). */
const FrameRecord *record_of(const Device &d, uint32_t frame_id)
{
	if (d.frame_counter == 0 || d.frames.empty()) return nullptr;
	/* ids are the low 32 bits of the frame counter: the newest frame that carries this one */
	const uint64_t newest = d.frame_counter - 1, id = newest - (uint32_t)((uint32_t)newest - frame_id);
	if (id > newest || newest - id >= d.frames.size()) return nullptr;
	const FrameRecord &f = d.frames[id % d.frames.size()];
	return (f.id == frame_id && !f.failed && f.bytes) ? &f : nullptr;
}

/* beamformer_hip_copy_frame: one frame by its id, as export_last_frames copies the newest ones; one device only */
bool copy_frame(uint32_t frame_id, void *out, uint64_t out_size)
{
	Context &c = g_context;
	if (!c.device_ready || c.device_count != 1) return set_error(BeamformerLibErrorKind_InvalidAccess);
	Device &d = c.devices[0];
	const FrameRecord *f = record_of(d, frame_id);
	if (!f || f->offset > d.ring.size || f->bytes > d.ring.size - f->offset) return set_error(BeamformerLibErrorKind_InvalidAccess);
	if (out_size < f->bytes) return set_error(BeamformerLibErrorKind_ExportSpaceOverflow);
	bool ok = HIP_OK(hipSetDevice(d.device));
	ok = ok && HIP_OK(hipMemcpyAsync(out, (const char *)d.ring.ptr + f->offset, f->bytes, hipMemcpyDeviceToHost, d.stream));
	ok = ok && HIP_OK(hipStreamSynchronize(d.stream));
	return ok || set_error(BeamformerLibErrorKind_InvalidAccess);
}

/* beamformer_hip_get_frame_info: beamformer_hip_get_last_frame_info for that id */
bool frame_info(uint32_t frame_id, BeamformerHipFrameInfo *out)
{
	Context &c = g_context;
	if (!c.device_ready || c.device_count != 1) return set_error(BeamformerLibErrorKind_InvalidAccess);
	const Device &d = c.devices[0];
	const FrameRecord *f = record_of(d, frame_id);
	if (!f) return set_error(BeamformerLibErrorKind_InvalidAccess);
	out->device_pointer = (char *)d.ring.ptr + f->offset;
	out->size_bytes = f->bytes;
	out->points[0] = f->points[0]; out->points[1] = f->points[1]; out->points[2] = f->points[2];
	out->data_kind = (uint32_t)f->data_kind;
	out->frame_id = f->id; out->parameter_block = f->block;
	return true;
}

} // namespace bf
