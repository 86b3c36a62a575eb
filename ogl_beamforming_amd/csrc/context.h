/* context.h -- process-global state of the in-process HIP beamformer.
 *
 * Stands where the reference has a server process: BeamformerCtx / BeamformerComputeContext
 * (beamformer_internal.h:386-470) reached through BeamformerSharedMemory
 * (beamformer_shared_memory.c:133-166).  Here the "server" is this library: parameter
 * blocks are plain host structs, the RF ring, the ping-pong buffers and the frame ring are
 * HIP device allocations, timelines are stream order + HIP events. */
#ifndef BF_CONTEXT_H
#define BF_CONTEXT_H

#include <hip/hip_runtime_api.h>
#include <cstdint>
#include <functional>
#include <string>
#include <list>
#include <vector>
#include "planner.h"
#include "bf_kernels.h"
#include "das_select.h"
#include "../../include/ogl_beamformer_hip.h"

namespace bf {

#define HIP_OK(expr) ((expr) == hipSuccess)
inline uint64_t round_up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }

struct DeviceBuffer {
	void  *ptr  = nullptr;
	size_t size = 0;
	bool ensure(size_t bytes);      /* grows (never shrinks); false on allocation failure */
	void release();
};

/* beamformer_internal.h:413-422 (BeamformerFrame / backlog) */
struct FrameRecord {
	uint64_t offset = 0, bytes = 0;
	uint32_t points[3]{1, 1, 1};
	int      data_kind = BeamformerDataKind_Float32;
	uint32_t id = 0, block = 0;
	int      timing_slot = -1;
	uint32_t tag = 0;                /* BeamformerViewPlaneTag of a views push's frame (0 for every other push, whose tag stops at validation as it always
	                                    has).  Recorded for the consumer the tag exists for -- a display that routes frames to its planes; no call reports it yet */
	bool     failed = false;         /* tombstone of a push that did not complete (executor.cpp, Tombstones) */
};

/* one RF frame in flight on the upload side (beamformer_rf_upload's slot, beamformer_core.c:1756-1805) */
struct UploadSlot {
	void      *pinned = nullptr;         /* hipHostMalloc staging the caller's bytes land in */
	size_t     pinned_size = 0;
	hipEvent_t copied = nullptr;         /* H2D of this slot finished (copy stream) */
	hipEvent_t consumed = nullptr;       /* the frame that read this slot's device buffers finished (compute stream) */
	bool       copy_pending = false, consume_pending = false;
	bool       unfenced_reader = false;  /* a frame read this slot's device buffers without recording `consumed` */
};

struct TimingSlot {
	hipEvent_t events[BEAMFORMER_HIP_MAX_TIMED_STAGES + 1]{};
	uint32_t   kinds[BEAMFORMER_HIP_MAX_TIMED_STAGES]{};
	uint32_t   count = 0;
	bool       created = false;
	bool       sampled = true;       /* false: this frame recorded no events; events_slot names the slot whose events stand in */
	uint32_t   events_slot = 0;
	uint32_t   share = 1;            /* frames the events of events_slot cover: a frame of a burst reports 1 / share of each time (push_frames) */
	uint64_t   das_voxels = 0;
	uint32_t   das_taps = 0, das_sample_bytes = 0, das_path = 0;
	bool       counted = false;
	uint64_t   frame_id = 0;
	uint64_t   violations_slot = ~0ull;   /* staged kernels: index of this frame's window-violation counter, or ~0 */
	uint32_t   das_row_end_planes = 0;    /* planes the row-end rule sent to the kernel behind the staged one */
	bool       failed = false;            /* the push that owns this slot did not complete */
};

/* the newest multi-frame push (executor.cpp push_frames, and the push_* function for its route): what the beamformer_hip_get_last_*_info calls report, each of its own kind */
struct PushRecord {
	enum Kind { None, Burst, Views, Image, BurstViews, Variants } kind = None;
	uint64_t      first_id = 0;
	uint32_t      count = 0, events_slot = 0;
	BurstDecision burst;                      /* Burst: its route */
	BeamformerHipViewsDescription views{};    /* Views: its route, and the host time spent deciding it */
	ReadiImageDecision image;                 /* Image: its route, and the RF frames it compounded */
	BeamformerHipBurstViewsDescription burst_views{};   /* BurstViews: its route; rf_frames RF frames on count / rf_frames views */
	BeamformerHipVariantsDescription variants{};        /* Variants: its route */
	uint32_t      rf_frames = 0;
	float         decide_us = 0;
	uint32_t      mixed = 0;                  /* frames that mix_last_frames / autocorrelate_last_frames / convolve_last_frames / warp_last_frames / queue_localisation_map / queue_track_map have queued behind the push: the push stays "the newest push" behind them */
};

struct PlanState {
	Plan         plan;
	bool         valid = false;
	DeviceBuffer hadamard_t, hadamard_base, readi_hadamard, transmits, sparse, mapping;
	std::vector<DeviceBuffer> taps;     /* per stage: filter taps (+ demodulation phasors) */
	std::list<std::vector<float>> tap_tables;   /* host copies the async uploads read from */
	uint64_t     generation = 0;          /* bumped by every successful commit (replan) of this block on this device */
	std::vector<BfTransmit>   transmit_table;
	std::vector<uint16_t>     readi_bits;
	std::string  error;
	std::vector<DasDecision> das_parts;   /* the DAS kernel(s) and geometry of this plan's frames (das_select.cpp: decide_das_parts), reused until
	                                         the plan, the shard, the path mode or a hook changes */
	uint32_t     das_z_first = 0, das_z_count = 0;
};

/* A READI image push's derived block (das_select.h: derive_readi_image) on one device: its plan state -- the transmit table of its
 * G x A transmits, the DAS decision -- kept with the block's own plan state and rebuilt when that one is (source_generation). */
struct ImagePlanState {
	PlanState      ps;
	ParameterBlock pb;
	uint64_t       source_generation = 0;
};

/* A variants push's derived block (das_select.h: derive_variant) on one device: the DAS decision of the block with `variant`'s three
 * values -- BfDasArgs, the part list, the staged / factored / HERCULES geometry planned with them -- kept with the block's own plan
 * state and reused while the triple, the block's plan (source_generation), the path mode and the hooks are what it was decided for; a
 * replan of the block drops them all.  The device tables a DAS launch reads besides (transmits, sparse elements, READI matrix) do not
 * depend on the triple: the derived state runs on the block's own (executor.cpp: Push::das_ps), and the tables the staged and HERCULES
 * kernels build per launch are built from the job's own BfDasArgs. */
struct VariantPlanState {
	DasVariant variant{};
	std::vector<DasDecision> parts;
	uint64_t   source_generation = 0, hooks_version = 0;
	uint32_t   mode = 0;
};
constexpr size_t kMaxVariantPlans = 256;          /* per block: four pushes of BEAMFORMER_HIP_MAX_VARIANTS; a push that would exceed it starts the list afresh */

constexpr uint32_t kTimingSlots = 32;    /* beamformer_compute_stats.c: 32-frame table */
constexpr uint32_t kStageIngest    = 0xFFFF;
constexpr uint32_t kStagePairCount = 0xFFFE;

constexpr uint32_t kMaxDevices = 8;      /* one node of MI355X */

/* The bytes of a run of `count` frames, contiguous in the frame ring, each rounded to 64 bytes: `count` frames of `points` voxels, or --
 * `views` given -- frame k of views[k]'s.  Host arithmetic only, saturating (three 32-bit extents can wrap 64 bits).  False: the run
 * does not fit `ring` bytes. */
inline bool frame_run_bytes(const uint32_t points[3], const BeamformerHipView *views, uint32_t count, uint64_t voxel_bytes, uint64_t ring, uint64_t &total,
                            uint32_t per_view = 1)
{
	/* equal frames: one size, `count` times; views: frame j is of views[j / per_view] (a burst views push: per_view RF frames a view) */
	const uint32_t distinct = views ? count / per_view : 1u, each = views ? per_view : count;
	total = 0;
	for (uint32_t k = 0; k < distinct; k++) {
		const uint32_t *n = views ? views[k].output_points : points;
		const uint64_t plane = (uint64_t)n[0] * n[1];
		if (plane > ring || plane * n[2] > ring / voxel_bytes) return false;
		const uint64_t frame = (plane * n[2] * voxel_bytes + 63) / 64 * 64;
		if (each && frame > (ring - total) / each) return false;
		total += frame * each;
	}
	return true;
}

/* The device state of the calls that work on frames already in the ring (frame_ops.cpp); all of it is created on first use. */
struct FrameOps {
	DeviceBuffer metrics_scratch;                              /* score_last_frames: the frames' BfMetricsRows, their results, the blocks' partials (frame_metrics.hip); find_peaks, accumulate_peaks, gram and correlate carve their tables from it too */
	void        *metrics_pinned = nullptr;                     /* ... the pinned memory the rows are sent from and the results land in (free again when the call returns: it ends in a synchronise) */
	size_t       metrics_pinned_size = 0;
	hipEvent_t   metrics_begin = nullptr, metrics_end = nullptr;   /* ... and the event pair around its launches, created once */
	DeviceBuffer peaks_list;                                   /* find_peaks_last_frames: the packed records of a call (frame_peaks.hip); its tables live in metrics_scratch and metrics_pinned */
	hipEvent_t   peaks_begin = nullptr, peaks_end = nullptr;   /* ... and the event pair around its emit launch (metrics_begin / metrics_end: around mark and scan) */
	/* A map the peak calls deposit into: `points` voxels of uint32 counts and, behind them from sums_at() on, `sum_components` times as
	 * many int64 sums (frame_peaks.hip, frame_tracks.hip deposit into it); points[0] == 0: none.  Beside it what the deposits since its
	 * reset add up to. */
	struct DepositMap {
		explicit DepositMap(uint32_t sums) : sum_components(sums) {}
		DeviceBuffer buffer;
		uint32_t     points[3]{};
		uint32_t     sum_components;                           /* 0 or 3 */
		uint32_t     calls = 0, block = 0;                     /* the successful calls that deposited since the reset, and the parameter block of the newest frame of the last one */
		uint64_t     pairs = 0, deposited = 0, outside = 0;    /* ... and their totals */
		uint64_t voxels() const { return (uint64_t)points[0] * points[1] * points[2]; }
		size_t   sums_at() const { return round_up(sizeof(uint32_t) * voxels(), 64); }
		size_t   bytes() const { return sum_components ? sums_at() + sum_components * sizeof(int64_t) * (size_t)voxels() : sizeof(uint32_t) * (size_t)voxels(); }
		bool     exists() const { return buffer.ptr && points[0]; }
		void     forget() { points[0] = points[1] = points[2] = 0; calls = block = 0; pairs = deposited = outside = 0; }   /* no map, nothing counted; the buffer stays */
		void     credit(uint32_t newest_block, uint64_t more_pairs, uint64_t more_deposited, uint64_t more_outside)      /* one successful call's deposits */
		{
			calls++; block = newest_block; pairs += more_pairs; deposited += more_deposited; outside += more_outside;
		}
	};
	DepositMap   map{0};                                       /* the localisation map: counts alone (beamformer_hip_localisation_map_reset) */
	DepositMap   tracks{3};                                    /* the track map: counts and three displacement sums (beamformer_hip_track_map_reset) */
	DeviceBuffer tracks_scratch;                               /* pair_peaks_last_frames, track_peaks_last_frames, draw_tracks_last_frames: what is sized by the peaks the scan found -- positions, choices, the match pass's tables and the pair records, or the chain tables and the track and point records, and the smoothed points (frame_tracks.hip); its small tables live in metrics_scratch and metrics_pinned, its peak records in peaks_list */
	DeviceBuffer mix_table;                                    /* mix_last_frames, autocorrelate_last_frames, convolve_last_frames, warp_last_frames: the source frames' ring offsets and the weight table (the tap table; the rotations and the field) of a call (ensemble.hip, autocorr.hip, spatial.hip, warp.hip) */
	void        *mix_pinned = nullptr;                         /* ... the pinned memory they are sent from, free again once mix_copied has passed (the call does not synchronise) */
	hipEvent_t   mix_copied = nullptr, mix_begin = nullptr, mix_end = nullptr;   /* ... and the event pair around its launch */
	bool         mix_copy_pending = false;
	DeviceBuffer blend_table;                                  /* mix_field_last_frames: the nodes' weight tables and the cell table of a call (ensemble_blocks.hip); the sources' ring offsets travel in mix_table */
	void        *blend_pinned = nullptr;                       /* ... the pinned memory they are sent from, grown on demand, free again once blend_copied has passed (the call does not synchronise) */
	size_t       blend_pinned_size = 0;
	hipEvent_t   blend_copied = nullptr;
	bool         blend_copy_pending = false;
	DeviceBuffer spatial_scratch;                              /* convolve_last_frames: what lies between two passes -- one run of frames, and the D fields of Normalised mode (spatial.hip) */
	void release();                                            /* everything above freed and as constructed; the caller has synchronised the device */
};

/* Everything that lives on one HIP device.  A process normally owns one (devices[0]); after
 * beamformer_hip_set_devices it owns several, each beamforming one z-slab of every frame. */
struct Device {
	int          device = -1;                                  /* HIP ordinal */
	uint32_t     index = 0;                                    /* position in Context::devices */
	hipStream_t  own_stream = nullptr, stream = nullptr;
	PlanState    plans[BeamformerMaxParameterBlocks];
	ImagePlanState image_plans[BeamformerMaxParameterBlocks];  /* READI image pushes: the derived FORCES block of plans[k] */
	std::list<VariantPlanState> variant_plans[BeamformerMaxParameterBlocks];   /* variants pushes: derived blocks of plans[k] */
	DeviceBuffer raw_staging[BeamformerMaxRawDataFramesInFlight];
	UploadSlot   upload[BeamformerMaxRawDataFramesInFlight];
	hipStream_t  copy_stream = nullptr;                        /* H2D of frame n+1 overlaps compute of frame n */
	DeviceBuffer rf[BeamformerMaxRawDataFramesInFlight];     /* beamformer.meta:8: 3 in flight */
	uint64_t     rf_index = 0;
	DeviceBuffer scratch[2];                                   /* ping-pong (reference: 3 slots of one buffer) */
	DeviceBuffer ring;                                         /* frame ring ("BeamformedData") */
	uint64_t     ring_next_offset = 0, frame_counter = 0;
	std::vector<FrameRecord> frames;                           /* BeamformerMaxBacklogFrames records */
	TimingSlot   timing[kTimingSlots];
	uint64_t     last_sampled_frame = 0;                       /* frame id whose events are the newest real ones */
	uint32_t     last_sampled_block = 0;
	bool         have_sample = false;
	uint64_t     replan_frame = 0;                             /* first frame of the current plan */
	DeviceBuffer pair_counter, minmax_scratch, sum_scratch;
	FrameOps     ops;                                          /* the calls on frames already in the ring (frame_ops.cpp) */
	DeviceBuffer burst_stage[2];                               /* a burst: the pre-DAS stages' outputs of every frame of a burst, stage by stage */
	PushRecord   multi;
	DeviceBuffer readi_decoded;                                /* a READI image push: the DAS input decoded across its acquisitions (readi_decode.hip), 64 spare bytes behind it */
	DeviceBuffer views_table;                                  /* a views push: the BfViewRows and the prefix table das_views.hip reads; a READI sweep, a READI image push: the frames' group ids */
	void        *views_pinned = nullptr;                       /* ... and the pinned memory they are sent from, free again once views_copied has passed */
	hipEvent_t   views_copied = nullptr;
	bool         views_copy_pending = false;
	DeviceBuffer hercules_pairs;                               /* das_hercules.hip: {sample, difference} copy of the DAS input (IQ, linear) */
	DeviceBuffer staged_tables;        /* das_staged.hip, wave-uniform transmit tables (bf_launch_das_staged_tables) */
	DeviceBuffer staged_violations;    /* das_staged*.hip: one counter per timing slot of window positions outside the staged window */
	DeviceBuffer hercules_table;                               /* das_hercules.hip: per-row lateral table, rebuilt per launch */
	/* multi-device frames (executor.cpp run_peers): the RF of slot k landed on this device / the frame
	 * that read slot k has finished */
	hipStream_t  peer_stream = nullptr;                        /* carries the copies INTO this device */
	hipEvent_t   rf_landed[BeamformerMaxRawDataFramesInFlight]{}, rf_consumed[BeamformerMaxRawDataFramesInFlight]{};
	bool         consumed_pending[BeamformerMaxRawDataFramesInFlight]{};
	uint32_t     slab_first = 0, slab_count = 0;               /* planes of the current multi-device frame */
	int          peer_access = 2;                              /* how RF reaches this device from devices[0]: 2 = it IS that device (or the ingest
	                                                              device itself), 1 = direct peer access over xGMI enabled, 0 = no peer access:
	                                                              hipMemcpyPeerAsync stages the copy through host memory */
	hipEvent_t   peer_copy_begin[BeamformerMaxRawDataFramesInFlight]{}, peer_copy_end[BeamformerMaxRawDataFramesInFlight]{};   /* timed */
	uint32_t     last_rf_slot = 0;                             /* RF slot of the newest frame */
	uint64_t     last_rf_bytes = 0;
	const void  *last_rf = nullptr;                            /* what the newest frame's first stage read: the library's own RF slot, never a caller's pointer */
	bool         last_rf_sum_ready = false;                    /* a borrowed device buffer: its checksum was taken inside the push */
	const void  *das_input = nullptr;                          /* what the newest push's DAS stage read (the RF slot, a scratch buffer or a burst's
	                                                              stage buffer; null: no DAS stage, or the push did not reach it), a frame's size,
	                                                              and -- a burst -- the frames it holds, das_input_stride bytes apart (one frame, or
	                                                              a views push's one input: stride 0) -- beamformer_hip_copy_das_input_frame */
	uint64_t     das_input_bytes = 0, das_input_stride = 0;
	uint32_t     das_input_frames = 0;
	uint64_t     das_decoded_bytes = 0;                        /* a READI image push: readi_decoded holds this many bytes of decoded DAS input, what
	                                                              beamformer_hip_copy_das_input serves (0: any other push) */
	/* frame graphs (beamformer_hip_enable_frame_graphs): one instantiated hipGraph per parameter block, updated
	 * in place from each frame's capture; graph_generation = the plan generation it was warmed up for */
	hipGraphExec_t frame_exec[BeamformerMaxParameterBlocks]{};
	uint64_t       graph_generation[BeamformerMaxParameterBlocks]{};
};

struct Context {
	/* library-level state that needs no device */
	BeamformerLibErrorKind last_error = BeamformerLibErrorKind_None;
	int32_t        timeout_ms = 0;
	ParameterBlock blocks[BeamformerMaxParameterBlocks];
	uint32_t       reserved_parameter_blocks = 1;              /* beamformer.c:249-263 */
	BeamformerLiveImagingParameters live{};
	uint32_t       live_dirty_flags = 0;
	uint64_t       frame_ring_bytes = 0;                       /* beamformed_frame_buffer_size */
	uint32_t       das_path_mode = 0;
	bool           count_pairs = false;
	bool           hilbert_enabled = false;                    /* beamformer_hip_enable_hilbert */
	bool           frame_graphs = false;                       /* beamformer_hip_enable_frame_graphs */
	uint64_t       graph_frames = 0, graph_instantiations = 0; /* frames replayed from a graph / graphs instantiated */

	/* device state */
	int          requested_devices[kMaxDevices]{-1, -1, -1, -1, -1, -1, -1, -1};
	uint32_t     requested_count = 0;                          /* 0: one device, chosen from the environment */
	bool         device_ready = false;
	Device       devices[kMaxDevices];
	uint32_t     device_count = 1;
	Device      *cur = &devices[0];                            /* the device the executor functions act on */
	std::vector<float> rf_time_deltas;
	double       last_push_time = 0;
	uint64_t     push_sequence = 0;                            /* id of the next frame, on EVERY device: one counter, so that the devices of
	                                                              beamformer_hip_set_devices stay in lockstep even after a push that failed half way */
};

Context &ctx();
bool     set_error(BeamformerLibErrorKind kind);   /* records and returns false */

/* executor.cpp */
bool ensure_device();                               /* SharedMemory error when no HIP device */
uint64_t default_frame_ring_bytes();
bool push_rf_and_compute(uint32_t block, const void *data, uint32_t size, bool data_on_device);
/* beamformer_hip_describe_upload: decide_upload's decision for `frames` raw frames of frame_size bytes each (one: the single push) */
bool describe_upload(const ParameterBlock &pb, const Plan &plan, uint64_t frame_size, uint32_t frames, const void *device_pointer,
                     BeamformerHipUploadDescription *out);
bool push_burst(uint32_t block, const void *data, uint32_t frame_size, uint32_t frame_count, const uint32_t *groups, bool data_on_device);   /* groups: a READI sweep */
bool push_readi_image(uint32_t block, const void *data, uint32_t frame_size, uint32_t frame_count, const uint32_t *groups, bool data_on_device);
bool last_readi_image_info(BeamformerHipReadiImageInfo *out);
void describe_readi_image_decision(const ReadiImageDecision &route, BeamformerHipReadiImageDescription *out);
bool last_burst_info(BeamformerHipBurstInfo *out);
void describe_burst_decision(const BurstDecision &route, BeamformerHipBurstDescription *out);
bool push_views(uint32_t block, const void *data, uint32_t size, const BeamformerHipView *views, uint32_t view_count, bool data_on_device);
bool last_views_info(BeamformerHipViewsInfo *out);
bool push_burst_views(uint32_t block, const void *data, uint32_t frame_size, uint32_t frame_count, const BeamformerHipView *views, uint32_t view_count,
                      bool data_on_device);
bool last_burst_views_info(BeamformerHipBurstViewsInfo *out);
bool push_variants(uint32_t block, const void *data, uint32_t size, const DasVariant *variants, uint32_t variant_count, bool data_on_device);
bool last_variants_info(BeamformerHipVariantsInfo *out);
void describe_variants_decision(const VariantsDecision &route, uint32_t variant_count, BeamformerHipVariantsDescription *out);
void describe_burst_views_decision(const BurstViewsDecision &route, uint32_t view_count, BeamformerHipBurstViewsDescription *out);
std::vector<ViewGrid> view_grids(const BeamformerHipView *views, uint32_t view_count);     /* the grids decide_views takes */
void describe_views_decision(const ViewsDecision &route, uint32_t view_count, BeamformerHipViewsDescription *out);
bool wait_for_frames(int32_t timeout_ms);
const FrameRecord *newest_record(const Device &d);     /* null: the newest push did not complete */
bool export_last_frames(void *out, uint64_t out_size, uint32_t count, int32_t timeout_ms);
bool last_frame_timings(BeamformerHipFrameTimings *out);
bool device_frame_timings(uint32_t device_index, BeamformerHipFrameTimings *out);
bool device_info(uint32_t device_index, BeamformerHipDeviceInfo *out);
bool fill_stats_table(BeamformerComputeStatsTable *out);
bool frame_min_max(float out[2]);
bool copy_das_input(void *out, uint64_t out_size);
bool copy_das_input_frame(uint32_t frame, void *out, uint64_t out_size);
bool sum_last_frames(uint32_t count, void *out, uint64_t out_size);
bool display_last_frame(float threshold_db, float gamma, float db_cutoff, float *out, uint64_t out_floats);
const FrameRecord *record_of(const Device &d, uint32_t frame_id);   /* null: no such frame, a tombstone, or storage that a newer frame reused */
bool copy_frame(uint32_t frame_id, void *out, uint64_t out_size);
bool frame_info(uint32_t frame_id, BeamformerHipFrameInfo *out);
void shutdown_device();
/* ... and for frame_ops.cpp: the ring side of a run of `count` frames of `points` voxels queued behind the newest frames -- where
 * the placement rule will put it, and the run itself: its ids taken and its frames placed, then enqueue(first id, first frame's record) */
bool queued_run_landing(const Device &d, const uint32_t points[3], uint32_t count, bool cplx, uint64_t &run_first, uint64_t &run_bytes);
bool claim_queued_run(Device &d, const uint32_t points[3], uint32_t tag, uint32_t count, bool cplx, uint32_t block,
                      const std::function<bool(uint64_t first, const FrameRecord &frame0)> &enqueue);

/* frame_ops.cpp */
/* What the five peak calls are asked in common (include/ogl_beamformer_hip.h has each member's meaning); the arguments arrive checked
 * (lib_api.cpp).  A call that takes no placements, reach or cap leaves them 0. */
struct PeakQuery {
	uint32_t count;
	const BeamformerHipFrameRegion *region;
	const float  *thresholds;  uint32_t threshold_count;               /* one for all frames, or one a frame */
	const double *placements;  uint32_t placement_count;               /* likewise: 12 numbers each */
	uint32_t use_offsets;
	float    max_distance;
	uint32_t max_per_frame;
	float threshold_of(uint32_t frame) const { return thresholds[threshold_count == 1 ? 0 : frame]; }
	const double *placement_of(uint32_t frame) const { return placements + (placement_count == 1 ? 0 : 12 * (size_t)frame); }
};
bool score_last_frames(uint32_t count, const BeamformerHipFrameRegion *region, BeamformerHipFrameMetrics *out, float *device_ms);
bool find_peaks_last_frames(const PeakQuery &q, BeamformerHipFramePeaks *frames, BeamformerHipFramePeak *peaks, uint32_t *peak_count,
                            float *device_ms);                     /* (no placements) */
bool quantiles_last_frames(uint32_t count, const BeamformerHipFrameRegion *region, const double *fractions, uint32_t fraction_count,
                           BeamformerHipFrameQuantiles *frames, BeamformerHipFrameQuantile *quantiles, uint32_t *histograms,
                           float *device_ms);                      /* arguments checked by the caller (lib_api.cpp) */
float peak_threshold_of(float value, bool cplx);                   /* host only; value finite and >= 0 (the caller checks) */
bool deposit_map_reset(FrameOps::DepositMap &map, const uint32_t points[3]);   /* ctx().devices[0].ops.map or .tracks; null: release; else checked by the caller */
bool accumulate_peaks_last_frames(const PeakQuery &q, BeamformerHipMapDeposits *frames, float *device_ms);
bool localisation_map_copy(uint32_t *out, uint64_t out_count, BeamformerHipMapInfo *info);
bool queue_localisation_map(float scale, uint32_t image_plane_tag, uint32_t *frame_id, float *device_ms);
bool pair_peaks_last_frames(const PeakQuery &q, uint32_t deposit, BeamformerHipPeakPairs *rows, BeamformerHipPeakPair *pairs, uint32_t *pair_count,
                            float *device_ms);
bool track_peaks_last_frames(const PeakQuery &q, uint32_t min_length, uint32_t deposit, BeamformerHipTrackedFrame *rows, BeamformerHipPeakTrack *tracks,
                             BeamformerHipTrackPoint *points, uint32_t *track_count, uint32_t *point_count, float *device_ms);
bool draw_tracks_last_frames(const PeakQuery &q, uint32_t min_length, uint32_t smooth, uint32_t deposit, BeamformerHipDrawnFrame *rows, float *device_ms);
bool track_map_copy(uint32_t *counts, int64_t *sums, uint64_t out_count, BeamformerHipTrackMapInfo *info);
bool queue_track_map(uint32_t component, float scale, uint32_t min_pairs, uint32_t image_plane_tag, uint32_t *frame_id, float *device_ms);
bool gram_last_frames(uint32_t count, const BeamformerHipFrameRegion *region, double *gram, BeamformerHipEnsembleInfo *info, float *device_ms);
bool correlate_last_frames(uint32_t count, uint32_t reference, const BeamformerHipFrameRegion *regions, uint32_t region_count,
                           const uint32_t max_shift[3], BeamformerHipShiftCorrelation *table, BeamformerHipCorrelationInfo *info, float *device_ms);
bool mix_last_frames(uint32_t count, const float *weights, uint32_t out_count, uint32_t image_plane_tag, uint32_t *first_frame_id,
                     float *device_ms);                            /* arguments checked by the caller (lib_api.cpp), but for what needs the frames' kind */
bool autocorrelate_last_frames(uint32_t count, const float *weights, uint32_t rows, uint32_t lag_count, uint32_t image_plane_tag,
                               uint32_t *first_frame_id, float *device_ms);   /* likewise; weights null: the identity form, rows == count */
bool convolve_last_frames(uint32_t count, const float *const taps[3], const uint32_t tap_counts[3], uint32_t mode, uint32_t image_plane_tag,
                          uint32_t *first_frame_id, float *device_ms);        /* likewise: the taps and the mode are checked by the caller */
bool warp_last_frames(uint32_t count, const float *field, const uint32_t nodes[3], const float node_first[3], const float node_step[3],
                      const float *rotations, uint32_t interpolation, uint32_t edge, uint32_t image_plane_tag,
                      uint32_t *first_frame_id, float *device_ms);            /* likewise: the field, the lattice and the modes are checked by the caller */
bool gram_boxes_last_frames(uint32_t count, const BeamformerHipFrameRegion *regions, uint32_t region_count, double *grams,
                            BeamformerHipEnsembleInfo *infos, float *device_ms);   /* likewise: the counts and the entry cap are checked by the caller */
void set_gram_boxes_budget(uint64_t bytes);                       /* hook GRAM_BOXES_BUDGET: the partials a batch of boxes may hold; 0: the default, BF_BLOCKS_BUDGET */
void set_blend_shape(int shape);                                 /* hook BLEND_SHAPE: 0 corners outermost, 1 sources once (where the lattice has no nodes along y), -1: the measured default */
bool mix_field_last_frames(uint32_t count, const float *weights, const uint32_t nodes[3], const uint32_t node_first[3],
                           const uint32_t node_step[3], uint32_t out_count, uint32_t image_plane_tag, uint32_t *first_frame_id,
                           float *device_ms);                      /* likewise: the counts, the lattice and the weights' finiteness are checked by the caller */

} // namespace bf
#endif
