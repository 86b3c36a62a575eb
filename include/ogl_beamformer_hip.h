/* ogl_beamformer_hip.h -- MI355X-specific additions to the C ABI of ogl_beamformer_lib.h.
 *
 * Nothing here exists in the reference library.  These entry points expose what an
 * in-process HIP backend can offer and the reference's shared-memory client cannot:
 * device selection, running on the caller's stream, RF that is already on the device
 * (e.g. landed by an RCCL broadcast over xGMI), sharding the output voxel grid across the
 * GPUs of a node (one process per GPU), device-side access to frames,
 * and per-stage timings taken with HIP events on the compute stream.
 *
 * Same conventions as ogl_beamformer_lib.h: returns 1 on success, 0 on failure with the
 * reason in beamformer_get_last_error().
 *
 * Threading: the library keeps one process-wide state (as the reference client keeps one
 * process-wide connection, lib/ogl_beamformer_lib.c:29-34) and takes no locks; call it from one
 * thread at a time.  Work it enqueues runs asynchronously on HIP streams; the data/compute
 * calls return before the frame is finished and beamformer_get_last_frames /
 * beamformer_hip_synchronize are the synchronisation points.
 */
#ifndef OGL_BEAMFORMER_HIP_H
#define OGL_BEAMFORMER_HIP_H

#include "ogl_beamformer_lib.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Select the HIP device the library owns.  Must precede the first call that touches the
 * device; afterwards it only succeeds for the device already in use.  Default: the value
 * of BEAMFORMER_HIP_DEVICE, else LOCAL_RANK, else 0. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_set_device(int32_t device_index);
BEAMFORMER_LIB_EXPORT int32_t  beamformer_hip_get_device(void);

/* Several devices behind the same push-RF / pull-image calls (the voxel grid shards,
 * the RF does not).  ONE process, `count` devices (1..8; HIP ordinals; the same ordinal may be listed more
 * than once, which is how a one-GPU box tests the path).  Must precede the first call that touches a
 * device; afterwards it only succeeds for the set already in use (beamformer_hip_shutdown releases it).
 *   - device_indices[0] is the ingest device: beamformer_push_data_with_compute /
 *     beamformer_hip_push_device_data_with_compute land the RF there exactly as with one device;
 *   - the channel-mapped RF is then copied to every other device (hipMemcpyPeerAsync over xGMI, one copy
 *     stream per destination, three RF slots deep so the copies of frame n+1 run beside the kernels of
 *     frame n) and each device runs the whole stage list on its own contiguous z-slab of the block's
 *     grid (of its output shard, if one is set): device i of n takes planes [i P / n, (i + 1) P / n) of
 *     the P planes.  No reduction collective -- voxels are independent (das.glsl:368-407);
 *   - beamformer_get_last_frames returns whole frames: the slabs stitched in z order, each frame rounded
 *     to 64 bytes exactly as one device exports it (lib/ogl_beamformer_lib.c:656-702 semantics);
 *     a slab is bit-identical to the same planes of a one-device frame;
 *   - beamformer_hip_frame_min_max combines the per-slab extremes on the host; the Sum and display
 *     reductions run per slab and are stitched the same way; beamformer_compute_timings reports, per
 *     stage, the slowest device; beamformer_hip_get_last_frame_info describes the ingest device's slab;
 *     beamformer_hip_set_stream is refused (a stream belongs to one device). */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_set_devices(const int32_t *device_indices, uint32_t count);
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_get_device_count(void);

/* Run all work on the caller's stream (a hipStream_t; 0 restores the library's own
 * stream).  Lets a host framework order its own device work (an RCCL broadcast of the RF
 * frame, a consumer of the image) against the beamformer without host synchronisation. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_set_stream(void *hip_stream);

/* Restrict the frames computed from a parameter block to the z-planes
 * [z_first, z_first + z_count) of its output grid; z_count == 0 restores the whole grid.
 * Voxel coordinates are still normalised by the WHOLE grid (das.glsl:374-376), so the planes
 * of a shard are bit-identical to the same planes of an unsharded frame.  Frames of a
 * sharded block hold X*Y*z_count voxels. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_set_output_shard(uint32_t parameter_slot,
                                                               uint32_t z_first, uint32_t z_count);

/* beamformer_push_data_with_compute() for RF that already resides on the library's device
 * (same layout and size rules).  The frame reads `device_data` on the library's current stream
 * -- in place by its first stage when no channel map / contrast reduction / row padding has to
 * be applied, through a copy into the RF ring otherwise; the caller may overwrite the buffer
 * from work it enqueues later on that stream, or after beamformer_hip_synchronize(). */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_push_device_data_with_compute(const void *device_data, uint32_t size,
                                                                            uint32_t image_plane_tag,
                                                                            uint32_t parameter_slot);

/* Block until every queued frame is complete. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_synchronize(void);

typedef struct {
	void    *device_pointer;    /* valid until the frame ring wraps over it */
	uint64_t size_bytes;        /* rounded up to 64, as exported by beamformer_get_last_frames */
	uint32_t points[3];         /* x, y, z (z = shard planes) */
	uint32_t data_kind;         /* BeamformerDataKind_Float32 or _Float32Complex */
	uint32_t frame_id;
	uint32_t parameter_block;
} BeamformerHipFrameInfo;
/* The newest frame, in place on the device (no copy, no synchronisation). */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_get_last_frame_info(BeamformerHipFrameInfo *out);

#define BEAMFORMER_HIP_MAX_TIMED_STAGES 24
typedef struct {
	uint32_t stage_count;
	uint32_t stage_kind[BEAMFORMER_HIP_MAX_TIMED_STAGES];  /* BeamformerShaderKind; ingest = 0xFFFF */
	float    stage_ms[BEAMFORMER_HIP_MAX_TIMED_STAGES];    /* hipEvent pairs on the compute stream */
	float    frame_ms;                                     /* first event to last event */
	uint64_t das_pairs;        /* (voxel, channel, transmit) triples passing the apodization
	                              test; counted only when pair counting is enabled */
	uint64_t das_voxels;
	uint32_t das_taps;         /* 1 nearest, 2 linear, 4 cubic */
	uint32_t das_sample_bytes; /* 4 real / 8 complex float32 */
	uint32_t das_path;         /* 0 general kernel, 1 separable-delay gather kernel, 2 LDS-staged kernel, 3 per-voxel factored kernel,
	                              4 HERCULES aligned-grid kernel, 5 factored kernel with block-wide LDS staging (das_tile.hip) */
	uint32_t staged_window_violations;   /* LDS-staged kernels with the STAGED_CHECKED hook: (wave, channel) pairs in which a term's position
	                                        fell outside the staged window -- the host's window bound was wrong.  Must be 0. */
	uint32_t tile_staged_chunks;         /* das path 5 (das_tile.hip): (block, chunk of four channels) pairs whose terms were read from the windows the
	                                        block staged in LDS ... */
	uint32_t tile_gather_chunks;         /* ... and those whose spread did not fit the window: the block ran das_factored.hip's gather loop for them */
	uint32_t das_row_end_planes;         /* z-planes of the frame the ROW-END rule handed to the kernel behind the staged one (LDS-staged -> gather /
	                                        factored; block-staged factored -> factored): planes on which a term can come within reach of an end of
	                                        its RF row, where sample_rf's range test is decided by the shader's own index, evaluated exactly
	                                        (csrc/das_exact.h).  0 on acquisitions whose rows do not end inside the image; das_path then names the
	                                        kernel that took the most planes */
} BeamformerHipFrameTimings;
/* Timings of the newest frame; waits for it to finish. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_get_last_frame_timings(BeamformerHipFrameTimings *out);

/* ---- bursts: N RF frames of one geometry per call (Flash / ULM ensembles: hundreds of frames from one parameter block) ----
 * frame_count RF frames back to back in `data`, each `frame_size` bytes under exactly the layout and size rules of
 * beamformer_push_data_with_compute; all beamformed with parameter block `parameter_slot`.  Queues frame_count frames: they
 * take consecutive frame ids, oldest = first in `data`, and beamformer_get_last_frames(out, size, frame_count) returns them.
 *   - one upload, one RF-ring slot (grown to hold the burst), one API call; the frames lie contiguously in the frame ring (a burst
 *     that would straddle its end starts again at offset 0);
 *   - RCA-family blocks (Flash, RCA_TPW, RCA_VLS) whose single frames run the general kernel take ONE DAS launch for the whole
 *     burst (csrc/das_burst.hip: a thread computes the geometry of each (channel, transmit) term once and applies it to
 *     BEAMFORMER_HIP_BURST_FRAMES_PER_THREAD frames); every other block runs its single-frame DAS kernel once per frame on that
 *     frame's slice of the batched DAS input.  beamformer_hip_describe_burst says which, and why;
 *   - the ingest and every pre-DAS stage run ONCE for the burst (the filters in chunks of 65535 / channel_count frames: the grid limit);
 *   - validation is the single push's, per frame, with the same error kinds; frame_count == 0 and frame_count >
 *     BEAMFORMER_HIP_MAX_BURST_FRAMES are BufferOverflow; frame_count == 1 IS the single push.  The burst must fit as a whole:
 *     frame_count x the 64-byte-rounded frame must not exceed the frame ring (FrameSizeOverflow) and the RF must fit device memory
 *     (RFDataSizeOverflow).  A burst that is refused queues nothing: no frame id is consumed.  A burst that fails after that leaves
 *     a tombstone under every one of its ids, as a failed single push does under its one;
 *   - every frame of a burst appears in beamformer_compute_timings and beamformer_hip_get_last_frame_timings with the burst's
 *     stage times divided by frame_count (one event set per burst);
 *   - several devices (beamformer_hip_set_devices, count > 1): refused with InvalidAccess -- a burst is not sharded; frame graphs:
 *     a burst runs as direct launches; pair counting: the geometry-only count runs once and every frame of the burst reports it; an
 *     output shard on the block is honoured. */
#define BEAMFORMER_HIP_MAX_BURST_FRAMES        1024u
#define BEAMFORMER_HIP_BURST_FRAMES_PER_THREAD 4u
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_push_data_burst_with_compute(const void *data, uint32_t frame_size, uint32_t frame_count,
                                                                           uint32_t image_plane_tag, uint32_t parameter_slot);
/* ... for RF that already resides on the library's device (beamformer_hip_push_device_data_with_compute's rules; a burst is always
 * copied or ingested into the RF ring, never read in place) */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_push_device_data_burst_with_compute(const void *device_data, uint32_t frame_size, uint32_t frame_count,
                                                                                  uint32_t image_plane_tag, uint32_t parameter_slot);

typedef struct {
	uint32_t burst_kernel;          /* 1: das_burst.hip takes the burst in das_launches launches; 0: the single-frame kernel(s), once per frame */
	int32_t  single_path;           /* the single-frame decision this was derived from (BeamformerHipFrameTimings::das_path numbering; -1 / -2 as
	                                   BeamformerHipDasDescription::path) */
	uint32_t frames_per_thread;     /* burst kernel: BEAMFORMER_HIP_BURST_FRAMES_PER_THREAD; else 1 */
	uint32_t das_launches;          /* DAS launches of the whole burst */
	uint32_t stage_launches;        /* launches the whole burst takes of a pre-DAS filter stage (1 up to 65535 / channel_count frames); the ingest, Decode, Reshape: 1 */
	uint32_t min_frames;            /* the smallest burst the burst kernel takes (csrc/das_select.h: kBurstMinFrames) */
	char     reason[160];           /* why this route */
} BeamformerHipBurstDescription;
/* What a burst of frame_count frames of a parameter block would run, under the current das path mode.  Needs no device. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_describe_burst(uint32_t parameter_slot, uint32_t frame_count, BeamformerHipBurstDescription *out);

typedef struct {
	BeamformerHipBurstDescription route;   /* of the burst that ran */
	uint32_t first_frame_id, frame_count;
	uint32_t stage_count;
	uint32_t stage_kind[BEAMFORMER_HIP_MAX_TIMED_STAGES];  /* BeamformerShaderKind; ingest = 0xFFFF */
	float    stage_ms[BEAMFORMER_HIP_MAX_TIMED_STAGES];    /* hipEvent pairs around each stage of the WHOLE burst */
	float    burst_ms;                                     /* first event to last event */
} BeamformerHipBurstInfo;
/* The newest burst (frame_count >= 2); waits for it to finish.  Fails when the newest push was not a burst or did not complete. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_get_last_burst_info(BeamformerHipBurstInfo *out);

/* ---- READI sweeps: the N group acquisitions of a READI sequence per call ----
 * A READI image is the sum of readi_group_count partial frames; acquisition k is beamformed with readi_group = g_k, which selects row
 * g_k of the Hadamard matrix as per-group signs (shaders/das.glsl:323-366).  A sweep is a burst with a group list: frame_count RF
 * frames back to back in `data` under exactly the burst's layout and size rules, and frame k is the frame a single push of RF k would
 * give if the block's readi_group were readi_groups[k].  readi_groups == NULL means (block.readi_group + k) % readi_group_count.
 * Everything else is the burst's contract (above):
 *   - consecutive frame ids, oldest = first in `data`; one upload and one RF-ring slot; the ingest and every pre-DAS stage ONCE; the
 *     frames contiguous in the frame ring; one event set, every frame reporting its 1 / frame_count share; an output shard on the block
 *     is honoured; several devices are refused (InvalidAccess); frame graphs: direct launches; pair counting: one count, reported by
 *     every frame; frame_count == 0 and frame_count > BEAMFORMER_HIP_MAX_BURST_FRAMES are BufferOverflow.  frame_count == 1 goes through
 *     the same code as any other count (it is NOT handed to the single push: its group comes from the list);
 *   - blocks whose single frames run the general kernel (every READI block on the automatic path) take ONE DAS launch for sweeps of
 *     min_frames frames and more (csrc/das_burst.hip: das_readi_burst_kernel -- a thread computes each (channel, transmit) term's
 *     geometry once and applies it to BEAMFORMER_HIP_BURST_FRAMES_PER_THREAD frames, each under its own group's signs); a frame of it
 *     is within float rounding of its single push and its bits do not depend on its place in the sweep.  Otherwise -- fewer frames,
 *     BeamformerHipDasPath_NoBurstKernel -- every frame runs the single-frame launch(es) with its group, and IS the single push's frame
 *     bit for bit.  beamformer_hip_describe_readi_sweep says which, and why;
 *   - refusals, all before a device is touched and before ids are taken (a refused sweep queues nothing): a block that is not READI --
 *     an acquisition kind other than FORCES / UFORCES, or readi_group_count <= 1 -- is InvalidAccess, with a line on stderr; a list
 *     entry >= readi_group_count is InvalidComputeStage, the kind a single push of a block with that readi_group gets (the planner
 *     refuses the block).  A sweep that fails later leaves tombstones under all its ids;
 *   - beamformer_hip_get_last_burst_info serves a sweep as it serves a burst (route.min_frames: the sweep's threshold).
 * The plain burst call keeps its behaviour for READI blocks: every frame under the block's one readi_group, on the per-frame route. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_push_data_readi_sweep_with_compute(const void *data, uint32_t frame_size, uint32_t frame_count,
                                                                                 const uint32_t *readi_groups, uint32_t image_plane_tag,
                                                                                 uint32_t parameter_slot);
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_push_device_data_readi_sweep_with_compute(const void *device_data, uint32_t frame_size, uint32_t frame_count,
                                                                                        const uint32_t *readi_groups, uint32_t image_plane_tag,
                                                                                        uint32_t parameter_slot);
/* What a sweep of frame_count frames would run, under the current das path mode (min_frames: csrc/das_select.h kReadiSweepMinFrames).
 * The block and the list are judged as the push judges them.  Needs no device. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_describe_readi_sweep(uint32_t parameter_slot, const uint32_t *readi_groups, uint32_t frame_count,
                                                                   BeamformerHipBurstDescription *out);
/* The group of every frame of such a sweep, as the push resolves the list (NULL included): out[frame_count].  Needs no device. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_resolve_readi_groups(uint32_t parameter_slot, const uint32_t *readi_groups, uint32_t frame_count,
                                                                   uint32_t *out);

/* ---- READI image: the N group acquisitions of a READI sequence compounded into ONE frame per call ----
 * The input is a READI sweep's exactly (above): frame_count RF frames back to back under the single push's layout and size rules,
 * readi_groups[k] the group of frame k, NULL meaning (block.readi_group + k) % readi_group_count.  The push queues ONE frame, with one
 * frame id.  DEFINITION of that frame: READI_FORCES is FORCES with transmit element tx_group * acquisition_count + tx_event and every
 * term multiplied by Hadamard[readi_group * G + tx_group] (shaders/das.glsl:288-366), and interpolation, IQ rotation, apodization and
 * accumulation are linear in the samples.  The image is therefore the frame a single push would give for the DERIVED BLOCK on the
 * DECODED ACQUISITION D:
 *     derived block   the same block with acquisition_kind = FORCES, acquisition_count = readi_group_count x acquisition_count, READI
 *                     off (UFORCES blocks with readi_group_count > 1 ignore sparse_elements in the shader: their derived block is the
 *                     same non-sparse FORCES block);
 *     D               D[channel][t * A + event][sample] = sum over k of H[g_k][t] * x_k[channel][event][sample], t < G, where x_k is
 *                     the DAS INPUT of RF frame k -- the decode takes place after every pre-DAS stage -- and the sum is float32,
 *                     k = 0, 1, ... frame_count - 1 in that order (csrc/readi_decode.hip).
 * It does G times less DAS work than the sweep (C x G x A terms a voxel instead of N x C x G x A) and needs no DAS arithmetic of its
 * own.  The list need not cover every group: an omitted group contributes nothing, a repeated one counts twice.  frame_count == 1 is
 * valid.
 *   - WITHOUT coherency weighting the image is the sum of the sweep's frame_count frames to within float rounding.
 *   - WITH coherency_weighting set the weighting is taken over ALL terms of the image -- FORCES' epilogue on D: (sum of all terms)
 *     x |sum of all terms| / (sum of every term's magnitude).  This is NOT the sum of separately weighted partial frames, which weights
 *     each acquisition by its own coherence; a caller who wants that sums the sweep's frames.
 *   - refusals, all before a device is touched and before an id is taken (a refused push queues nothing): a block that is not READI
 *     (kind other than FORCES / UFORCES, or readi_group_count <= 1) InvalidAccess with a line on stderr; a list entry >=
 *     readi_group_count InvalidComputeStage; frame_count == 0 or > BEAMFORMER_HIP_MAX_BURST_FRAMES BufferOverflow; readi_group_count x
 *     acquisition_count > BeamformerMaxEmissionsCount InvalidAccess with a line on stderr; a decoded input of 4 GiB or more, or memory
 *     that cannot be grown, RFDataSizeOverflow; a frame larger than the frame ring FrameSizeOverflow; several devices InvalidAccess.
 *     A push that fails after its id is taken leaves a tombstone under it;
 *   - one upload and one RF-ring slot; the ingest and every pre-DAS stage ONCE for all RF frames, as for a sweep; then the decode; then
 *     the derived block's own single-frame DAS launch(es) -- its own decision (beamformer_hip_describe_das of the derived block), row-end
 *     rule included.  An output shard is honoured; frame graphs: direct launches; pair counting counts on the derived block;
 *   - the stage list of the push (beamformer_hip_get_last_readi_image_info, the frame's timing row) holds the across-acquisition
 *     decode as one extra entry of kind BeamformerShaderKind_Decode directly before DAS;
 *   - beamformer_hip_copy_das_input after an image push returns D, [channel][G x A][das_samples];
 *     beamformer_hip_copy_das_input_frame(k) for k < frame_count returns x_k, what the decode read;
 *   - beamformer_hip_get_last_burst_info and beamformer_hip_get_last_views_info refuse an image push. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_push_data_readi_image_with_compute(const void *data, uint32_t frame_size, uint32_t frame_count,
                                                                                 const uint32_t *readi_groups, uint32_t image_plane_tag,
                                                                                 uint32_t parameter_slot);
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_push_device_data_readi_image_with_compute(const void *device_data, uint32_t frame_size, uint32_t frame_count,
                                                                                        const uint32_t *readi_groups, uint32_t image_plane_tag,
                                                                                        uint32_t parameter_slot);
typedef struct {
	uint32_t transmit_count;        /* the derived block's acquisition_count: readi_group_count x acquisition_count */
	int32_t  das_path;              /* the derived block's own DAS decision (BeamformerHipDasDescription::path numbering, -1 / -2 included) */
	uint32_t das_launches;          /* DAS launches of the push: the derived block's single-frame launches, once */
	uint32_t stage_launches;        /* launches the push takes of a pre-DAS filter stage (BeamformerHipBurstDescription::stage_launches) */
	uint32_t decode_launches;       /* launches of the across-acquisition decode: 1 (0: no DAS kernel runs) */
	char     reason[160];
} BeamformerHipReadiImageDescription;
/* What an image push of frame_count RF frames would run, under the current das path mode; the block, the list and the count are judged
 * as the push judges them.  Needs no device. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_describe_readi_image(uint32_t parameter_slot, const uint32_t *readi_groups, uint32_t frame_count,
                                                                   BeamformerHipReadiImageDescription *out);
typedef struct {
	BeamformerHipReadiImageDescription route;   /* of the push that ran */
	uint32_t frame_id, rf_frame_count;
	uint32_t stage_count;
	uint32_t stage_kind[BEAMFORMER_HIP_MAX_TIMED_STAGES];  /* BeamformerShaderKind; ingest = 0xFFFF; the across-acquisition decode: Decode, directly before DAS */
	float    stage_ms[BEAMFORMER_HIP_MAX_TIMED_STAGES];    /* hipEvent pairs around each stage of the WHOLE push */
	float    image_ms;                                     /* first event to last event */
} BeamformerHipReadiImageInfo;
/* The newest image push; waits for it to finish.  Fails when the newest push was not an image push or did not complete. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_get_last_readi_image_info(BeamformerHipReadiImageInfo *out);

/* ---- views: ONE RF frame beamformed on K voxel grids per call (live X-plane / tri-plane imaging: the reference's 3DXPlane view;
 * ULM patch refinement: tens to hundreds of small fine grids around detections, all from the RF of one push) ----
 * `data` is one RF frame under exactly the layout and size rules of beamformer_push_data_with_compute.  Everything except the grid
 * comes from parameter block `parameter_slot`: view k is the frame a single push of the same RF would give if the block's
 * das_voxel_transform and output_points[0..2] were views[k]'s.  Queues view_count frames: they take consecutive frame ids in view
 * order, and beamformer_get_last_frames(out, size, view_count) returns them oldest first, each at its own 64-byte-rounded size.
 *   - one upload, one RF-ring slot, ONE launch of the ingest and of every pre-DAS stage; the views lie contiguously in the frame ring,
 *     each rounded to 64 bytes (a run that would straddle the end of the ring starts again at offset 0);
 *   - every view gets its own single-frame decision (beamformer_hip_describe_das's, on that grid).  Views of RCA-family blocks
 *     (Flash, RCA_TPW, RCA_VLS) that the general kernel would run take ONE DAS launch together (csrc/das_views.hip: the tiles of all
 *     such views side by side along the grid, each block the general kernel's own loop on its view's grid, no channel split) when
 *     their 256-voxel tiles number at least BeamformerHipViewsDescription::min_tiles; every other view runs its single-frame kernel(s)
 *     on the shared DAS input.  A view's bits do not depend on which other views the push holds, nor on their order.
 *     beamformer_hip_describe_views says which route, and why;
 *   - beamformer_hip_get_last_frame_info describes the LAST view (its points); every frame record carries its view's points and tag;
 *   - validation is the single push's, with the same error kinds (DataSizeMismatch, InvalidImagePlane per view,
 *     ParameterBlockUnallocated, ...).  view_count == 0 and view_count > BEAMFORMER_HIP_MAX_VIEWS are BufferOverflow; views == NULL or
 *     a zero extent is InvalidAccess; all views together (each rounded to 64 bytes) exceeding the frame ring is FrameSizeOverflow;
 *     several devices (beamformer_hip_set_devices, count > 1) or an output shard on the block is InvalidAccess -- a view is not
 *     sharded.  Everything that can be refused is checked before a device is touched, and every buffer whose absence
 *     would fail the push is grown before the ids are taken: a refused push queues nothing.  A push that fails after that leaves a tombstone under every one of its ids;
 *   - view_count == 1 goes through the same code (it is not the single push: the grid comes from the view);
 *   - one event set per push: every view appears in beamformer_compute_timings and beamformer_hip_get_last_frame_timings with the
 *     push's stage times divided by view_count; frame graphs: a views push runs as direct launches; pair counting: the
 *     geometry-only count runs per view. */
#define BEAMFORMER_HIP_MAX_VIEWS 1024u
typedef struct {
	float    das_voxel_transform[16];   /* as BeamformerParameters::das_voxel_transform (column major) */
	uint32_t output_points[3];          /* x, y, z voxels of this view, each >= 1 */
	uint32_t image_plane_tag;           /* BeamformerViewPlaneTag */
} BeamformerHipView;
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_push_data_views_with_compute(const void *data, uint32_t size, const BeamformerHipView *views,
                                                                           uint32_t view_count, uint32_t parameter_slot);
/* ... for RF that already resides on the library's device (beamformer_hip_push_device_data_with_compute's rules; the RF of a views
 * push is always ingested into the RF ring, never read in place) */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_push_device_data_views_with_compute(const void *device_data, uint32_t size, const BeamformerHipView *views,
                                                                                  uint32_t view_count, uint32_t parameter_slot);

typedef struct {
	uint32_t kernel_views;          /* views das_views.hip takes, all in one launch (0: none) */
	uint32_t das_launches;          /* DAS launches of the whole push: that one, plus the single-frame launch(es) of every other view */
	uint32_t min_tiles;             /* the fewest 256-voxel tiles of eligible views the views kernel takes (csrc/das_select.h: kViewsMinTiles) */
	int8_t   path[BEAMFORMER_HIP_MAX_VIEWS];   /* per view: its OWN single-frame decision (BeamformerHipFrameTimings::das_path numbering; -1 / -2 as
	                                              BeamformerHipDasDescription::path), whichever route the push takes */
	char     reason[160];           /* why this route */
} BeamformerHipViewsDescription;
/* What a views push of these grids on a parameter block would run, under the current das path mode.  Needs no device. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_describe_views(uint32_t parameter_slot, const BeamformerHipView *views, uint32_t view_count,
                                                             BeamformerHipViewsDescription *out);

typedef struct {
	BeamformerHipViewsDescription route;   /* of the push that ran */
	uint32_t first_frame_id, view_count;
	uint32_t stage_count;
	uint32_t stage_kind[BEAMFORMER_HIP_MAX_TIMED_STAGES];  /* BeamformerShaderKind; ingest = 0xFFFF */
	float    stage_ms[BEAMFORMER_HIP_MAX_TIMED_STAGES];    /* hipEvent pairs around each stage of the WHOLE push */
	float    views_ms;                                     /* first event to last event */
	float    decide_us;                                    /* host time the push spent deciding its views' routes */
} BeamformerHipViewsInfo;
/* The newest views push; waits for it to finish.  Fails when the newest push was not a views push or did not complete. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_get_last_views_info(BeamformerHipViewsInfo *out);

/* ---- burst views: N RF frames of one geometry beamformed on K voxel grids per call (bi-plane / tri-plane ultrafast imaging with a
 * row-column array: the X-plane view over a Flash or few-angle ensemble; ULM: an ensemble refined on one set of patches) ----
 * `data` is the burst's: frame_count RF frames back to back, each `frame_size` bytes under exactly the layout and size rules of
 * beamformer_push_data_with_compute; `views` is the views push's.  Frame (view v, RF frame k) is the frame a single push of RF k would
 * give if the block's das_voxel_transform and output_points[0..2] were views[v]'s.  Queues frame_count x view_count frames, VIEW-MAJOR:
 * frame v * frame_count + k is (view v, RF frame k), so a view's ensemble is frame_count consecutive ids -- in the frame ring
 * frame_count equal-sized frames at a fixed stride --, the views' runs follow one another, each frame rounded to 64 bytes (a run that
 * would straddle the end of the ring starts again at offset 0), and beamformer_get_last_frames(out, size, frame_count x view_count)
 * returns them oldest first, each at its own size.
 *   - one upload, one RF-ring slot, the ingest and every pre-DAS stage ONCE for the push (the burst's frame chunks), one event set:
 *     every frame's timing row shows a 1 / (frame_count x view_count) share; beamformer_hip_copy_das_input_frame(k) serves RF frame k;
 *   - the DAS route is a ladder (csrc/das_select.h: decide_burst_views; beamformer_hip_describe_burst_views says which rung, and why):
 *       1. frame_count >= BeamformerHipBurstViewsDescription::min_frames, neither NoBurstKernel (0x400) nor NoViewsKernel (0x800):
 *          the views a views push's kernel is eligible for (RCA family, single frames on the general kernel) run in ONE launch whatever
 *          their tile count (csrc/das_burst.hip: das_burst_views_kernel -- the burst kernel's frame slots on the views kernel's
 *          concatenated tiles); every other view runs its single-frame kernel(s) per RF frame.  A frame of the fused launch is within
 *          float rounding of its single push (the burst kernel's contract); its bits depend neither on its slot nor on the other views;
 *       2. below the threshold, or under 0x400: per RF frame the views push's own DAS step -- frame (v, k) is the frame of a views
 *          push of RF k alone, bit for bit;
 *       3. under 0x800, and for every view rung 1 does not take: the view's single-frame launch(es) per RF frame -- frame (v, k) is
 *          the single push of RF k on the block with that grid, bit for bit;
 *   - validation is the single push's per frame and the views push's per view, with their error kinds.  frame_count == 0 or >
 *     BEAMFORMER_HIP_MAX_BURST_FRAMES, view_count == 0 or > BEAMFORMER_HIP_MAX_VIEWS, and frame_count x view_count >
 *     BeamformerMaxBacklogFrames (every frame keeps its record) are BufferOverflow; views == NULL or a zero extent is InvalidAccess;
 *     the whole run exceeding the frame ring is FrameSizeOverflow; RF or stage memory that cannot be grown is RFDataSizeOverflow;
 *     several devices or an output shard on the block is InvalidAccess.  All of that is judged before a device is touched and before
 *     an id is taken: a refused push queues nothing.  A push that fails after that leaves a tombstone under every one of its ids;
 *   - frame_count == 1 goes through the same code (rung 2 or 3);
 *   - beamformer_hip_get_last_burst_info, _views_info and _readi_image_info refuse this push, and its own info call refuses theirs;
 *     frame graphs: the push runs as direct launches; pair counting: one geometry-only count per view, reported by all of that view's
 *     frames; das path flag FailViewsDas (0x2000) fails this push's DAS step as it fails a views push's. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_push_data_burst_views_with_compute(const void *data, uint32_t frame_size, uint32_t frame_count,
                                                                                 const BeamformerHipView *views, uint32_t view_count,
                                                                                 uint32_t parameter_slot);
/* ... for RF that already resides on the library's device (beamformer_hip_push_device_data_burst_with_compute's rules) */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_push_device_data_burst_views_with_compute(const void *device_data, uint32_t frame_size, uint32_t frame_count,
                                                                                        const BeamformerHipView *views, uint32_t view_count,
                                                                                        uint32_t parameter_slot);

typedef struct {
	uint32_t rung;                  /* 1, 2 or 3: the lowest-numbered rung some view of the push runs on (above) */
	uint32_t kernel_views;          /* rung 1: views the fused kernel takes, all in one launch; else 0 */
	uint32_t frame_kernel_views;    /* rung 2: views das_views.hip takes, once per RF frame; else 0 */
	uint32_t das_launches;          /* DAS launches of the whole push */
	uint32_t stage_launches;        /* launches the push takes of a pre-DAS filter stage (BeamformerHipBurstDescription::stage_launches) */
	uint32_t frames_per_thread;     /* rung 1: BEAMFORMER_HIP_BURST_FRAMES_PER_THREAD; else 1 */
	uint32_t min_frames;            /* the fewest RF frames the fused kernel takes (csrc/das_select.h: kBurstViewsMinFrames) */
	int8_t   path[BEAMFORMER_HIP_MAX_VIEWS];   /* per view: its OWN single-frame decision, as BeamformerHipViewsDescription::path */
	char     reason[160];           /* why this route */
} BeamformerHipBurstViewsDescription;
/* What a burst views push of frame_count RF frames on these grids would run, under the current das path mode.  Needs no device. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_describe_burst_views(uint32_t parameter_slot, uint32_t frame_count, const BeamformerHipView *views,
                                                                   uint32_t view_count, BeamformerHipBurstViewsDescription *out);

typedef struct {
	BeamformerHipBurstViewsDescription route;   /* of the push that ran */
	uint32_t first_frame_id, frame_count, view_count;      /* frame_count: RF frames; the push queued frame_count x view_count frames */
	uint32_t stage_count;
	uint32_t stage_kind[BEAMFORMER_HIP_MAX_TIMED_STAGES];  /* BeamformerShaderKind; ingest = 0xFFFF */
	float    stage_ms[BEAMFORMER_HIP_MAX_TIMED_STAGES];    /* hipEvent pairs around each stage of the WHOLE push */
	float    push_ms;                                      /* first event to last event */
	float    decide_us;                                    /* host time the push spent deciding its route (one decision per view, not per frame) */
} BeamformerHipBurstViewsInfo;
/* The newest burst views push; waits for it to finish.  Fails when the newest push was not one or did not complete. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_get_last_burst_views_info(BeamformerHipBurstViewsInfo *out);

/* ---- variants: ONE RF frame beamformed under K sets of DAS scalars per call (sound-speed autofocus, system-delay calibration, f-number
 * tuning: the same RF under K candidate values, the sharpest or most coherent result kept) ----
 * `data` is one RF frame under exactly the layout and size rules of beamformer_push_data_with_compute.  Everything except the three
 * values comes from parameter block `parameter_slot`: frame k is the frame a single push of the same RF would give if the block's
 * speed_of_sound, time_offset and f_number were variants[k]'s (time_offset is the BLOCK field, BeamformerParameters::time_offset: the
 * delays of the block's filters are added to it exactly as the planner adds them to the block's own).  Queues variant_count frames of
 * the block's own grid: they take consecutive frame ids, variant 0 first, lie contiguously in the frame ring (a run that would straddle
 * the end of the ring starts again at offset 0), and beamformer_get_last_frames(out, size, variant_count) returns them oldest first.
 *   - one upload, one RF-ring slot, ONE launch of the ingest and of every pre-DAS stage: only the DAS stage depends on the candidate;
 *   - the parameter block is left alone: no field is written, no dirty bit set, no replan -- a single push afterwards gives the block's
 *     own frame;
 *   - every variant gets its own single-frame decision (beamformer_hip_describe_das's, of the block carrying its values).  Variants of
 *     RCA-family blocks (Flash, RCA_TPW, RCA_VLS) that the general kernel would run take ONE DAS launch together (csrc/das_variants.hip:
 *     grid x the 256-voxel tiles of the grid, grid y the variant, each block the general kernel's own loop under its variant's values, no
 *     channel split) when variants x tiles number at least BeamformerHipVariantsDescription::min_tiles or the variants at least
 *     ::min_variants (the launch has a floor of about 36 us: it pays from 8 candidates, or 4 on a full 256 x 256 plane); such a frame is within float
 *     rounding of its single push, and its bits depend neither on the other variants nor on their order.  Every other variant -- other
 *     families, grids on which a faster kernel runs, planes the row-end rule cuts -- runs its single-frame kernel(s) on the shared DAS
 *     input under its own derived plan state, and IS the single push's frame bit for bit.  beamformer_hip_describe_variants says which
 *     route, and why;
 *   - validation is the single push's, with the same error kinds.  variant_count == 0 and variant_count > BEAMFORMER_HIP_MAX_VARIANTS
 *     are BufferOverflow; variants == NULL, a field that is not finite or speed_of_sound <= 0 is InvalidAccess (with a line on stderr);
 *     several devices (beamformer_hip_set_devices, count > 1) or an output shard on the block is InvalidAccess, as for a views push; the
 *     frames together exceeding the frame ring is FrameSizeOverflow; device memory that cannot be grown is RFDataSizeOverflow.  All of
 *     that is judged before a device is touched and before an id is taken: a refused push queues nothing.  A push that fails after that
 *     leaves a tombstone under every one of its ids (das path flag FailViewsDas, 0x2000, fails this push's DAS step as it fails a views
 *     push's);
 *   - variant_count == 1 goes through the same code;
 *   - one event set per push: every variant appears in beamformer_compute_timings and beamformer_hip_get_last_frame_timings with the
 *     push's stage times divided by variant_count; frame graphs: the push runs as direct launches; pair counting: the geometry-only
 *     count runs per variant (f_number changes it);
 *   - beamformer_hip_get_last_burst_info, _views_info, _burst_views_info and _readi_image_info refuse this push, and
 *     beamformer_hip_get_last_variants_info refuses theirs. */
#define BEAMFORMER_HIP_MAX_VARIANTS 64u
typedef struct {
	float speed_of_sound;               /* m/s, > 0 */
	float time_offset;                  /* s, as BeamformerParameters::time_offset */
	float f_number;
} BeamformerHipDasVariant;
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_push_data_variants_with_compute(const void *data, uint32_t size, const BeamformerHipDasVariant *variants,
                                                                              uint32_t variant_count, uint32_t image_plane_tag, uint32_t parameter_slot);
/* ... for RF that already resides on the library's device (beamformer_hip_push_device_data_with_compute's rules; the RF of a variants
 * push is always ingested into the RF ring, never read in place) */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_push_device_data_variants_with_compute(const void *device_data, uint32_t size,
                                                                                     const BeamformerHipDasVariant *variants, uint32_t variant_count,
                                                                                     uint32_t image_plane_tag, uint32_t parameter_slot);

typedef struct {
	uint32_t kernel_variants;       /* variants das_variants.hip takes, all in one launch (0: none) */
	uint32_t fused_launches;        /* launches of das_variants.hip: 1 or 0 */
	uint32_t das_launches;          /* DAS launches of the whole push: that one, plus the single-frame launch(es) of every other variant */
	uint32_t kernel_tiles;          /* blocks of the fused launch: kernel_variants x the grid's 256-voxel tiles */
	uint32_t min_tiles;             /* the variants kernel takes the eligible variants when variants x tiles reach this (csrc/das_select.h: kVariantsMinTiles) */
	uint32_t min_variants;          /* ... or when they number at least this (kVariantsMinVariants) */
	int8_t   path[BEAMFORMER_HIP_MAX_VARIANTS];    /* per variant: its OWN single-frame decision (BeamformerHipFrameTimings::das_path numbering; -1 / -2
	                                                  as BeamformerHipDasDescription::path), whichever route the push takes */
	uint8_t  taken[BEAMFORMER_HIP_MAX_VARIANTS];   /* per variant: 1 = in the fused launch */
	char     reason[160];           /* why this route */
} BeamformerHipVariantsDescription;
/* What a variants push of these candidates on a parameter block would run, under the current das path mode.  Needs no device and leaves
 * the block as it is. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_describe_variants(uint32_t parameter_slot, const BeamformerHipDasVariant *variants, uint32_t variant_count,
                                                                BeamformerHipVariantsDescription *out);

typedef struct {
	BeamformerHipVariantsDescription route;   /* of the push that ran */
	uint32_t first_frame_id, variant_count;
	uint32_t stage_count;
	uint32_t stage_kind[BEAMFORMER_HIP_MAX_TIMED_STAGES];  /* BeamformerShaderKind; ingest = 0xFFFF */
	float    stage_ms[BEAMFORMER_HIP_MAX_TIMED_STAGES];    /* hipEvent pairs around each stage of the WHOLE push */
	float    variants_ms;                                  /* first event to last event */
	float    decide_us;                                    /* host time the push spent deciding its variants' routes */
} BeamformerHipVariantsInfo;
/* The newest variants push; waits for it to finish.  Fails when the newest push was not a variants push or did not complete. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_get_last_variants_info(BeamformerHipVariantsInfo *out);

/* ---- frame metrics: the `count` newest frames of the frame ring reduced ON THE DEVICE to one small row of focus metrics each (the K
 * frames of a variants push scored so that the sharpest can be kept; the patches of a views push; per-frame energy and peak position
 * of a burst) -- instead of downloading them all to obtain `count` numbers ----
 * DEFINITION of a row (tests/frame_metrics_ref.py restates it in numpy).  The magnitude |v| of a voxel is ONE float32:
 * sqrtf(re * re + im * im) for Float32Complex frames, every operation rounded to float32 on its own (no fused multiply-add), fabsf(v)
 * for Float32 frames.  A voxel is finite when that float is.  Everything else is formed in double from that float: a = (double)|v|;
 * the powers a, a * a and (a * a) * (a * a); the gradient term d = (double)|v[i + 1]| - (double)|v[i]|, then d * d.  A voxel that is not
 * finite counts in non_finite and contributes to nothing else; a pair with such a voxel is not a pair; pairs never leave the box.
 * The sums are double sums in an order the box alone fixes (no floating-point atomics): the bits of a frame's row depend on that frame
 * and the region only -- not on count, not on the other frames of the call, not on the call being repeated. */
#define BEAMFORMER_HIP_MAX_SCORED_FRAMES 1024u      /* = BEAMFORMER_HIP_MAX_VIEWS: a whole views push can be scored */
typedef struct { uint32_t first[3], count[3]; } BeamformerHipFrameRegion;   /* a box of voxel indices, x, y, z; every count >= 1 */
typedef struct {
	uint32_t frame_id, parameter_block, data_kind, image_plane_tag;   /* from the frame's record */
	uint32_t points[3];                       /* the frame's own grid */
	uint32_t region_first[3], region_count[3];/* the box that was reduced (the whole frame when region == NULL) */
	uint32_t max_index[3];                    /* x, y, z IN THE FRAME (not relative to the box) of max_abs; the lowest flat index (x fastest) among ties;
	                                             0, 0, 0 when voxels == 0 */
	uint64_t voxels;                          /* voxels of the box whose magnitude is finite: the ones every sum below runs over */
	uint64_t non_finite;                      /* voxels of the box whose magnitude is NaN or infinite (coherency weighting leaves NaN where no term passed) */
	uint64_t gradient_pairs[3];               /* per axis: neighbour pairs (i, i + 1 along that axis) with both voxels inside the box and both finite */
	double   sum_abs, sum_abs2, sum_abs4;     /* sum of |v|, |v|^2, |v|^4 */
	double   gradient2[3];                    /* per axis: sum over those pairs of (|v[i + 1]| - |v[i]|)^2 */
	float    max_abs;                         /* largest finite |v|; 0 when voxels == 0 */
	uint32_t reserved;                        /* 0 (the struct has no padding: rows compare byte for byte) */
} BeamformerHipFrameMetrics;
/* out[count], oldest first (the order of beamformer_get_last_frames).  The frames may differ in grid and in data kind (a views push:
 * K sizes); every row carries its own points.  region == NULL: every frame whole; else the same box of every frame.  The reduction --
 * one partial launch for all frames, one launch that folds them (csrc/frame_metrics.hip) -- is enqueued on the library's current stream
 * behind the frames it reads (no host wait for them first); the rows come back through one device-to-host copy and one stream
 * synchronise.  device_ms, when not NULL: the time between two events around the two launches.
 * Refusals, all decided before anything is launched and leaving `out` unwritten: count == 0 or > BEAMFORMER_HIP_MAX_SCORED_FRAMES is
 * BufferOverflow; InvalidAccess: out == NULL; no device in use yet; fewer than count frames ever queued; one of the count frames a
 * tombstone (a push that did not complete), or its record overwritten, or its ring storage reused by a newer frame; a region with a
 * zero count, or one that does not fit inside EVERY one of the frames; several devices (beamformer_hip_set_devices: a frame is a set
 * of z-slabs there and the z gradient would cross them). */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_score_last_frames(uint32_t count, const BeamformerHipFrameRegion *region,
                                                                BeamformerHipFrameMetrics *out, float *device_ms);
/* The frame with this id -- while its record and its ring storage are still its own -- copied to host memory at its 64-byte-rounded
 * size, as beamformer_get_last_frames exports it: on the current stream, ending in a synchronise.  (beamformer_get_last_frames serves
 * the newest `count` only: this is how candidate k of a variants push is kept without downloading the ones behind it.)  An unknown
 * id, a tombstone, reused storage, out == NULL, no device yet, several devices: InvalidAccess; out_size below the rounded size:
 * ExportSpaceOverflow. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_copy_frame(uint32_t frame_id, void *out, uint64_t out_size);
/* beamformer_hip_get_last_frame_info for that id: in place, no copy, no synchronisation.  Refused as beamformer_hip_copy_frame. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_get_frame_info(uint32_t frame_id, BeamformerHipFrameInfo *out);

typedef enum {
	BeamformerHipFrameScore_Energy         = 0,   /* sum_abs2 */
	BeamformerHipFrameScore_MeanMagnitude  = 1,   /* sum_abs / voxels                       (speckle brightness) */
	BeamformerHipFrameScore_Sharpness      = 2,   /* voxels * sum_abs4 / sum_abs2^2         (normalised fourth moment) */
	BeamformerHipFrameScore_GradientEnergy = 3,   /* (gradient2[0] + [1] + [2]) / sum_abs2 */
	BeamformerHipFrameScore_Count
} BeamformerHipFrameScore;
/* Host only: touches no device and no library state but the last error.  scores[i] (scores may be NULL): the criterion of
 * metrics[i] as written above, evaluated in double; a row with voxels == 0 or sum_abs2 == 0 scores -INFINITY.  *best_index: the
 * highest score, the lowest index among ties.  Returns 0 (InvalidAccess) for count == 0, a NULL argument other than scores, an unknown criterion, or
 * when every score is -INFINITY (scores, when given, is filled all the same). */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_rank_frames(const BeamformerHipFrameMetrics *metrics, uint32_t count, uint32_t criterion,
                                                          double *scores, uint32_t *best_index);

/* ---- frame peaks: the local maxima of the `count` newest frames, found ON THE DEVICE (ULM: a burst push beamforms an ensemble on a
 * coarse grid; its peaks say where the 16 x 16-voxel patches of the burst views push that refines it go -- coarse ensemble -> peaks ->
 * patches -> refined ensemble without a frame leaving the device) ----
 * DEFINITION (tests/frame_peaks_ref.py restates it in numpy).  Every decision is taken on ONE float32 a voxel, the decision value q:
 * re * re + im * im for Float32Complex frames, every operation rounded to float32 on its own (no fused multiply-add), fabsf(v) for
 * Float32 frames.  No square root takes part in a decision, so numpy reproduces every one by basic IEEE operations.  A voxel is finite
 * when q is.  It is ELIGIBLE when it is finite and q >= t: t is `threshold` for real frames and the float32 product
 * threshold * threshold for complex ones -- the threshold is on the magnitude, in the frame's own units.  A voxel at flat frame index
 * i (x fastest) is a PEAK when it is eligible, lies inside the box, and for every voxel n of its 3 x 3 x 3 neighbourhood whose q_n is
 * finite: q > q_n when n's flat index is below i, q >= q_n when it is above.  The neighbourhood is clipped to the FRAME, not to the box:
 * a voxel on a face of the box is judged by its real neighbours, so tiling a frame into boxes neither invents nor doubles a peak.
 * Neighbours outside the frame and non-finite ones (the NaN coherency weighting leaves) do not count.  Under the tie rule no two
 * adjacent voxels are both peaks; of a plateau, the voxel of the lowest flat index is one (an all-zero frame at threshold 0: one peak,
 * at 0, 0, 0).
 * A record's magnitude is the frame metrics' magnitude of the voxel (sqrtf(q) for complex frames, q for real ones).  Axis a is FITTED
 * when both neighbours at -1 and +1 along it lie in the frame and are finite and den = (m_minus + m_plus) - (m0 + m0) is negative; then
 * offset[a] = 0.5f * (m_minus - m_plus) / den clamped to [-0.5, 0.5] -- the vertex of the parabola through the three magnitudes, in
 * voxels, float32 arithmetic in this operation order without contraction.  Axes that are not fitted carry 0.
 * A frame's list is in ascending flat frame index and depends on that frame, the box and the threshold only: not on count, not on the
 * other frames of the call, not on the call being repeated (the device uses no atomics: a peak's place is a function of its index). */
#define BEAMFORMER_HIP_MAX_PEAKS_PER_FRAME 65536u
typedef struct {
	uint32_t index[3];                        /* x, y, z IN THE FRAME */
	float    magnitude;
	float    offset[3];                       /* sub-voxel offset per axis, in voxels, within [-0.5, 0.5]; 0 where not fitted */
	uint32_t fitted;                          /* bit a: axis a was fitted */
} BeamformerHipFramePeak;                     /* 32 bytes, no padding */
typedef struct {
	uint32_t frame_id, parameter_block, data_kind, image_plane_tag;   /* from the frame's record */
	uint32_t points[3];                       /* the frame's own grid */
	uint32_t region_first[3], region_count[3];/* the box that was searched (the whole frame when region == NULL) */
	float    threshold;                       /* the threshold used for this frame */
	uint32_t first;                           /* index into `peaks` of this frame's first record */
	uint32_t stored;                          /* min(found, max_per_frame) */
	uint64_t found;                           /* every peak of the box, stored or not */
	uint64_t above_threshold;                 /* eligible voxels of the box */
} BeamformerHipFramePeaks;                    /* 80 bytes, no padding */
/* frames[count], oldest first; the frames may differ in grid and in data kind.  thresholds: threshold_count == 1: one for all frames;
 * else threshold_count == count, oldest first; each finite and >= 0.  `peaks` has room for count * max_per_frame records and comes back
 * PACKED: frame n's `stored` records start at frames[n].first, the frames follow one another, *peak_count is their total.  When
 * found > stored the records kept are the first in flat order: raise the threshold or the cap.  The call runs on the library's current
 * stream behind the frames it reads: the rows go up, a mark pass and a scan run (csrc/frame_peaks.hip), the per-frame counts come back
 * (first synchronise), the list buffer is grown to the total stored, the emit pass runs (skipped when the total is 0) and exactly the
 * stored records come back (second synchronise).  device_ms, when not NULL: the time between events around the launches, both parts
 * added.
 * Refusals, all decided before anything is launched and leaving every output unwritten: count == 0 or > BEAMFORMER_HIP_MAX_SCORED_FRAMES,
 * max_per_frame == 0 or > BEAMFORMER_HIP_MAX_PEAKS_PER_FRAME: BufferOverflow; InvalidAccess: a NULL pointer other than region and
 * device_ms; threshold_count neither 1 nor count; a threshold that is negative or not finite; and everything
 * beamformer_hip_score_last_frames refuses -- no device in use yet, fewer than count frames queued, a tombstone, an overwritten record,
 * reused storage, a region that does not fit inside every frame, several devices. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_find_peaks_last_frames(uint32_t count, const BeamformerHipFrameRegion *region,
                                                                     const float *thresholds, uint32_t threshold_count, uint32_t max_per_frame,
                                                                     BeamformerHipFramePeaks *frames, BeamformerHipFramePeak *peaks,
                                                                     uint32_t *peak_count, float *device_ms);
/* Host only: touches no device and no library state but the last error.  out[peak_count]: for every peak, the view of a views or
 * burst views push that is a patch of patch_points voxels spanning patch_extent_voxels SOURCE voxels around it.  source_voxel_transform
 * and source_points are those of the grid the peaks were found on.  The kernels map voxel i of an axis to i / max(1, points - 1) and
 * then through the transform M; per axis a, with P = source_points[a]: the normalised centre is c = (index + offset) / max(1, P - 1)
 * (offset dropped when use_offsets == 0) and the span s = extent / max(1, P - 1).  The patch's transform has the translation
 * M (c - s/2, 1) and column a of M times s where patch_points[a] > 1; where patch_points[a] == 1 -- its only index is 0 -- column a
 * of M unchanged (the matrix stays regular) and c in the place of c - s/2: patch voxel j of axis a lands on the source's fractional voxel
 * index + offset - extent/2 + j * extent / (patch_points[a] - 1).  InvalidAccess: a NULL argument, a zero patch_points entry, an extent
 * that is negative or not finite.  peak_count == 0 writes nothing and succeeds. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_peaks_to_views(const float source_voxel_transform[16], const uint32_t source_points[3],
                                                             const BeamformerHipFramePeak *peaks, uint32_t peak_count,
                                                             const uint32_t patch_points[3], const float patch_extent_voxels[3],
                                                             uint32_t use_offsets, uint32_t image_plane_tag, BeamformerHipView *out);

/* ---- frame quantiles: exact order statistics of the `count` newest frames, selected ON THE DEVICE where the frames lie, in the units the
 * peak calls decide in (a threshold from "the brightest 0.1 % of voxels are candidates" or "6 x the median" instead of a fraction of
 * max_abs, the single brightest voxel and the likeliest outlier; the range of a display between two percentiles; a scale for
 * beamformer_hip_queue_localisation_map) -- instead of downloading every frame to sort it ----
 * DEFINITION (tests/frame_quantiles_ref.py restates it in numpy).
 * DECISION VALUE.  The decision value q of a voxel is the one beamformer_hip_find_peaks_last_frames decides on: re * re + im * im for
 * Float32Complex frames, every operation rounded to float32 on its own (no fused multiply-add), fabsf(v) for Float32 frames.  No
 * square root takes part.  A voxel is finite when q is; a voxel that is not counts in non_finite and in nothing else.  q is never
 * negative and never -0, so the order of the values is the order of their bit patterns as uint32.
 * ORDER STATISTICS.  Let n be the finite voxels of the box and q_(0) <= ... <= q_(n-1) their decision values in ascending order.  A
 * fraction f is a double with 0 <= f <= 1.  Its rank is r = (uint64)floor(f * (double)(n - 1) + 0.5): one double multiply, one add,
 * one floor, no fused multiply-add -- numpy float64 reproduces it.  The quantile's `value` is q_(r), an actual voxel's value: nothing
 * is interpolated, so it is exact.  below = #{q < value} and equal = #{q == value}, so below <= r < below + equal.  When n == 0:
 * rank = below = equal = 0 and value = magnitude = threshold = 0.
 * MAGNITUDE AND THRESHOLD are formed on the host from `value`, so they are IEEE-exact.  magnitude is sqrtf(value) for complex frames
 * and value for real ones.  threshold is the number to hand to the peak calls: value for real frames; for complex frames the LARGEST
 * float32 T >= 0 with fl(T * T) <= value (what stepping from sqrtf(value) with nextafterf arrives at: the condition holds for T and
 * fails for the next float up).  With it the eligible set of beamformer_hip_find_peaks_last_frames (q >= fl(T * T)) contains every
 * voxel with q >= value; it contains nothing else unless a voxel's q lies in [fl(T * T), value).  Not every float is the rounded
 * square of a float, so equality with `value` cannot be promised.
 * COARSE HISTOGRAM (optional): BEAMFORMER_HIP_QUANTILE_BINS uint32 counts a frame; bin b counts the finite voxels of the box whose q
 * has bits >> 20 == b: 8 bins an octave of q, about 0.75 dB a bin for real frames and 0.38 dB for complex ones.  Bins from 2040 up are
 * the non-finite patterns and stay 0.  It is the first selection pass's table, handed out as it is.
 * Every count is an integer sum (the device adds with integer atomics, and no floating-point atomic exists in the library): the bytes
 * of a frame's rows and of its histogram depend on that frame, the region and the fractions only -- not on count, not on the other
 * frames of the call, not on the call being repeated. */
#define BEAMFORMER_HIP_MAX_QUANTILES  16u
#define BEAMFORMER_HIP_QUANTILE_BINS  2048u
typedef struct {
	double   fraction;                        /* as given */
	uint64_t rank, below, equal;
	float    value, magnitude, threshold;
	uint32_t reserved;                        /* 0 */
} BeamformerHipFrameQuantile;                 /* 48 bytes, no padding */
typedef struct {
	uint32_t frame_id, parameter_block, data_kind, image_plane_tag;   /* from the frame's record */
	uint32_t points[3];                       /* the frame's own grid */
	uint32_t region_first[3], region_count[3];/* the box that was ranked (the whole frame when region == NULL) */
	uint32_t first, stored, reserved;         /* this frame's records: quantiles[first .. first + stored), stored == fraction_count; reserved 0 */
	uint64_t voxels, non_finite;              /* finite / not finite voxels of the box */
} BeamformerHipFrameQuantiles;                /* 80 bytes, no padding */
/* frames[count], oldest first; the frames may differ in grid and in data kind, as for beamformer_hip_score_last_frames.  fractions
 * [fraction_count] need not be sorted and may repeat; quantiles[count * fraction_count] is frame-major, in the order of `fractions`.
 * histograms: NULL, or room for count * BEAMFORMER_HIP_QUANTILE_BINS counts, frame-major.  The call runs on the library's current stream
 * behind the frames it reads: the rows and the fractions go up in one copy, one memset zeroes the count tables, three count passes
 * each followed by a pick run (csrc/frame_quantiles.hip: a radix select on bits 30..20, 19..10 and 9..0 of q, so the frames are read
 * three times), the results come back in one copy -- the histograms in one more -- behind ONE stream synchronise.  device_ms, when not
 * NULL: the time between two events around the memset and the six launches.
 * Refusals, all decided before anything is enqueued and leaving every output unwritten: count == 0 or > BEAMFORMER_HIP_MAX_SCORED_FRAMES,
 * fraction_count == 0 or > BEAMFORMER_HIP_MAX_QUANTILES: BufferOverflow; InvalidAccess: fractions, frames or quantiles NULL; a
 * fraction that is NaN or outside [0, 1]; a box of more than 2^32 - 1 voxels; and everything beamformer_hip_score_last_frames refuses --
 * no device in use yet, fewer than count frames queued, a tombstone, an overwritten record, reused storage, a region that does not fit
 * inside every frame, several devices. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_quantiles_last_frames(uint32_t count, const BeamformerHipFrameRegion *region,
                                                                    const double *fractions, uint32_t fraction_count,
                                                                    BeamformerHipFrameQuantiles *frames /* [count] */,
                                                                    BeamformerHipFrameQuantile *quantiles /* [count * fraction_count] */,
                                                                    uint32_t *histograms /* [count][2048], may be NULL */, float *device_ms);
/* Host only: touches no device and no library state but the last error.  *threshold: the `threshold` of a quantile whose `value` is
 * decision_value, as defined above -- decision_value itself for BeamformerDataKind_Float32, the largest float32 T >= 0 with
 * fl(T * T) <= decision_value for BeamformerDataKind_Float32Complex.  InvalidAccess: threshold NULL, a decision value that is negative
 * or not finite, any other data kind. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_peak_threshold_of(float decision_value, uint32_t data_kind, float *threshold);

/* ---- localisation map: the peaks of the frames of the frame ring accumulated ON THE DEVICE into one grid of counts (ULM's product: the
 * sub-voxel positions of the peaks of thousands of frames binned on a grid several times finer than the beamforming grid -- no peak list
 * leaves the device, and the map can be queued into the frame ring as an ordinary Float32 frame, so that
 * beamformer_hip_convolve_last_frames (the Gaussian that renders it), beamformer_hip_display_last_frame,
 * beamformer_hip_score_last_frames, beamformer_hip_find_peaks_last_frames and beamformer_hip_copy_frame work on it) ----
 * The library holds ONE map: points[0] x points[1] x points[2] uint32 counts, x fastest, on the one device.
 * DEFINITION (tests/localisation_ref.py restates it in numpy).
 * PEAKS.  A voxel of a frame is a peak exactly when beamformer_hip_find_peaks_last_frames says so: the same decision value, thresholds,
 * box and frame-clipped neighbourhood (the same mark pass runs).  There is no cap: every found peak takes part.
 * POSITION.  A peak's position is its record, bit for bit what beamformer_hip_find_peaks_last_frames would have stored (one text
 * computes both): p_a = (double)index[a] + (double)offset[a] per axis, the offset dropped when use_offsets == 0.
 * PLACEMENT.  placements[n] is frame n's row-major 3 x 4 matrix A of doubles (placement_count == 1: one for all frames); the peak's
 * map coordinate is, per row r, in double, every product and every sum one operation of its own (no fused multiply-add), in this order:
 *     m_r = ((A[r][3] + A[r][0] * p_x) + A[r][1] * p_y) + A[r][2] * p_z
 * -- numpy float64 reproduces every bit.  Map voxel j of an axis has its centre at map coordinate j.
 * BIN.  b_r = floor(m_r + 0.5).  The peak is DEPOSITED when 0 <= b_r < points[r] on all three axes: the count at flat index
 * (b_z * points[1] + b_y) * points[0] + b_x goes up by 1.  Otherwise (a coordinate that is not a number included) it counts in `outside`
 * and nothing is written.
 * COUNTS are uint32 and WRAP at 2^32 (4 x 10^9 peaks in one bin: reset or read the map before).  Integer additions commute, so the
 * bytes of the map depend on the multiset of deposits since the reset only -- not on count, on the order of the calls or of the frames,
 * or on a call being split in two: the device adds with integer atomics, and no floating-point atomic exists in the library. */
#define BEAMFORMER_HIP_MAX_MAP_VOXELS (1u << 28)
/* points[3] (x fastest), each >= 1, product <= BEAMFORMER_HIP_MAX_MAP_VOXELS: (re)allocates the library's one map and zeroes it on the
 * current stream; its totals (BeamformerHipMapInfo) start again.  points == NULL releases it (always succeeds).
 * beamformer_hip_shutdown releases it too.  Starts the device when none is in use yet.  A zero extent: InvalidAccess; a product above
 * the limit: BufferOverflow; memory that cannot be allocated: RFDataSizeOverflow (then there is no map); several devices: InvalidAccess. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_localisation_map_reset(const uint32_t points[3]);
typedef struct {
	uint32_t frame_id, parameter_block, data_kind, image_plane_tag;   /* from the frame's record */
	uint32_t points[3];                       /* the frame's own grid */
	uint32_t region_first[3], region_count[3];/* the box that was searched (the whole frame when region == NULL) */
	float    threshold;                       /* the threshold used for this frame */
	uint32_t reserved[2];                     /* 0 (the second word stands where a compiler would pad: rows compare byte for byte) */
	uint64_t found, above_threshold;          /* exactly beamformer_hip_find_peaks_last_frames' numbers */
	uint64_t deposited, outside;              /* found == deposited + outside */
} BeamformerHipMapDeposits;                   /* 96 bytes, no padding */
/* The peaks of the `count` newest frames (count <= BEAMFORMER_HIP_MAX_SCORED_FRAMES), oldest first, deposited into the map.  region,
 * thresholds and threshold_count are beamformer_hip_find_peaks_last_frames'; the frames may differ in grid and in data kind, which is
 * why every frame may have its own placement (beamformer_hip_map_placement makes one from two voxel transforms).  frames[count] (may
 * be NULL): a row a frame.  The call runs on the library's current stream behind the frames it reads: the rows and the placements go up
 * in one copy, the mark pass and the scan run, then the deposit -- the mark pass's grid again: a block without a peak leaves after one
 * load, a lane that holds a peak forms its record, places it and adds 1 with one integer atomic -- and the scan again over the blocks'
 * tallies (csrc/frame_peaks.hip); the per-frame numbers come back in one copy behind ONE stream synchronise.  device_ms, when not NULL:
 * the time between two events around the four launches.
 * Refusals, all decided before anything is enqueued or changed and leaving every output unwritten: count == 0 or >
 * BEAMFORMER_HIP_MAX_SCORED_FRAMES: BufferOverflow; InvalidAccess: thresholds or placements NULL; threshold_count or placement_count
 * neither 1 nor count; a threshold that is negative or not finite; a placement entry that is not finite; no map (never reset, or
 * released); and everything beamformer_hip_score_last_frames refuses -- no device in use yet, fewer than count frames queued, a
 * tombstone, an overwritten record, reused storage, a region that does not fit inside every frame, several devices. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_accumulate_peaks_last_frames(uint32_t count, const BeamformerHipFrameRegion *region,
                                                                           const float *thresholds, uint32_t threshold_count,
                                                                           const double *placements /* [placement_count][12] */,
                                                                           uint32_t placement_count /* 1 or count */, uint32_t use_offsets,
                                                                           BeamformerHipMapDeposits *frames /* [count], may be NULL */,
                                                                           float *device_ms);
typedef struct {
	uint32_t points[3];
	uint32_t calls;                           /* successful beamformer_hip_accumulate_peaks_last_frames calls, and beamformer_hip_track_peaks_last_frames or beamformer_hip_draw_tracks_last_frames calls with BEAMFORMER_HIP_TRACK_DEPOSIT_POINTS, since the reset */
	uint64_t deposited, outside;              /* their totals */
} BeamformerHipMapInfo;                       /* 32 bytes, no padding */
/* The map's counts as they are, copied to out[out_count] behind everything enqueued on the current stream (one synchronise); *info
 * (may be NULL): the grid and the totals since the reset.  out NULL, no map, no device, several devices: InvalidAccess; out_count below
 * the map's voxel count: ExportSpaceOverflow. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_localisation_map_copy(uint32_t *out, uint64_t out_count, BeamformerHipMapInfo *info);
/* Queues ONE Float32 frame of the map's grid into the frame ring: each value (float)count * scale -- one unsigned-to-float conversion
 * rounded to nearest, then one float32 multiply.  The map itself is left unchanged.  The frame is placed, numbered, recorded and timed
 * exactly as a run of one frame of beamformer_hip_mix_last_frames is, the record of the newest multi-frame push (it stays "the newest
 * push" behind the frame) and *frame_id (may be NULL) included; its record carries image_plane_tag and the parameter block of the
 * newest frame of the most recent successful beamformer_hip_accumulate_peaks_last_frames call.  One launch (csrc/frame_peaks.hip) on
 * the current stream; the call does not synchronise unless device_ms is not NULL (then: the time between two events around the launch).
 * Refusals, all decided before anything changes: a scale that is not finite, no map, no device, several devices, no successful
 * accumulate call since the reset: InvalidAccess; a frame of the map's size that does not fit the ring: FrameSizeOverflow. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_queue_localisation_map(float scale, uint32_t image_plane_tag, uint32_t *frame_id, float *device_ms);
/* Host only: touches no device and no library state but the last error.  out[12]: the row-major 3 x 4 placement that takes a voxel
 * position of a frame (index + offset) to the map coordinate of the same point in space.  The kernels map voxel i of an axis with P
 * points to i / max(1, P - 1) and then through the column-major voxel transform M (see beamformer_hip_peaks_to_views); of M the upper
 * three rows are used (an affine map: linear part L, translation t).  With S = diag(1 / max(1, P_a - 1)):
 *     out = S_map^-1 L_map^-1 [ L_frame S_frame | t_frame - t_map ]      in double.
 * A planar map (an axis of one point) still needs a regular L_map: give that axis a non-zero extent -- its only voxel is index 0, and
 * a frame point at the axis's origin lands on it.  A rigid correction of a frame (beamformer_hip_displacements_from_correlation: frame
 * k shown at v + d is the reference at v) is a translation the caller adds to that frame's placement: out[4 r + 3] -= sum over a of
 * out[4 r + a] * d_a.
 * InvalidAccess: a NULL argument; a points entry 0; a singular map transform -- det L_map not finite, or |det| <= 10^-12 times the
 * product of the lengths of L_map's columns (a zero extent is the common case) --; a result that is not finite. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_map_placement(const float frame_voxel_transform[16], const uint32_t frame_points[3],
                                                            const float map_voxel_transform[16], const uint32_t map_points[3], double out[12]);

/* ---- peak pairs: the peaks of consecutive frames of the frame ring linked ON THE DEVICE, and the track map (what ULM publishes besides
 * the density of detections: the velocity map, and the rejection of detections that do not persist from one frame to the next --
 * instead of downloading every peak list through beamformer_hip_find_peaks_last_frames and pairing on the host, every ensemble) ----
 * The library holds ONE track map next to the localisation map, on the one device: points[0] x points[1] x points[2] uint32 counts and
 * three int64 displacement sums a voxel, x fastest.
 * DEFINITION (tests/tracks_ref.py restates it in numpy).  Every decision is integer or double arithmetic in a fixed operation order
 * without fused multiply-add: numpy float64 and int64 reproduce every bit.
 * PEAKS.  A frame's peaks are exactly the records of beamformer_hip_find_peaks_last_frames for the same frame, box, threshold and
 * max_per_frame (the same mark, scan and emit passes run: one text computes both).  A peak's RANK is its place in that list, in
 * ascending flat index; when found > max_per_frame the peaks kept are the first in flat order, as there.
 * POSITION.  p_a = (double)index[a] + (double)offset[a], the offset dropped when use_offsets == 0; the map coordinate, per row r of the
 * frame's row-major 3 x 4 double placement A (placement_count == 1: one for all frames), is
 *     m_r = ((A[r][3] + A[r][0] * p_x) + A[r][1] * p_y) + A[r][2] * p_z
 * -- the localisation map's formula, byte for byte.  A peak with any m_r not finite is UNPLACED: neither a query nor a candidate.
 * DISTANCE.  For a in frame n (the older) and b in frame n + 1: d_r = m_r(b) - m_r(a) and d2 = ((d_x * d_x) + (d_y * d_y)) + (d_z * d_z);
 * both directions use this one expression, so their bits agree.  b is WITHIN REACH of a when d2 <= R2, with
 * R2 = (double)max_distance * (double)max_distance formed once on the host; max_distance is in map coordinates.
 * CHOICE.  f(a) is the b within reach that minimises (d2, rank of b) lexicographically, g(b) the a within reach that minimises
 * (d2, rank of a); either is "none" when nothing is within reach.  The minimum is lexicographic, so it does not depend on the order in
 * which candidates are visited.
 * PAIR.  (a, b) is a pair of frame pair n when f(a) = b and g(b) = a: a peak is in at most one pair per neighbouring frame.  The pairs
 * of frame pair n are listed in ascending rank of a.  The lists depend on those two frames, the box, the thresholds, the placements and
 * max_distance only: not on count, not on the other frames of the call, not on the call being repeated (the device emits them without
 * atomics: a pair's place is a function of a).
 * DEPOSIT (deposit != 0).  The midpoint c_r = 0.5 * (m_r(a) + m_r(b)), its bin b_r = floor(c_r + 0.5).  Inside the track map on all
 * three axes: the bin's uint32 count goes up by 1 and its three int64 sums by q_r = (int64)floor(d_r * 1048576.0 + 0.5) (2^-20 of a map
 * voxel; |d_r| <= 2^20, so q_r fits by far); both WRAP.  Otherwise the pair counts in `outside` and nothing is written.  The device
 * adds with integer atomics, 32-bit for the count and 64-bit for the sums; integer additions commute, so the map's bytes are a function
 * of the multiset of deposits since the reset.  There is still no floating-point atomic in the library.
 * COST.  P_n x P_{n+1} distance evaluations a direction a frame pair, P the stored peaks of a frame: every peak of one frame is compared
 * with every peak of the other.  There is no search window and no spatial structure: bound P with the threshold and max_per_frame. */
#define BEAMFORMER_HIP_MAX_TRACK_MAP_VOXELS  (1u << 26)
#define BEAMFORMER_HIP_MAX_PAIR_DISTANCE     1048576.0f
#define BEAMFORMER_HIP_TRACK_MAP_COMPONENTS  5u
/* points[3] (x fastest), each >= 1, product <= BEAMFORMER_HIP_MAX_TRACK_MAP_VOXELS: (re)allocates the library's one track map (28 bytes
 * a voxel) and zeroes it on the current stream; its totals (BeamformerHipTrackMapInfo) start again.  points == NULL releases it (always
 * succeeds).  beamformer_hip_shutdown releases it too.  Starts the device when none is in use yet.  The error kinds are those of
 * beamformer_hip_localisation_map_reset: a zero extent: InvalidAccess; a product above the limit: BufferOverflow; memory that cannot be
 * allocated: RFDataSizeOverflow (then there is no map); several devices: InvalidAccess. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_track_map_reset(const uint32_t points[3]);
typedef struct {
	uint32_t frame;                           /* n: the frame pair, a in frame n of the call, b in frame n + 1 */
	uint32_t a, b;                            /* ranks: indices into the two frames' find_peaks lists */
	uint32_t deposited;                       /* 1: added to the track map; 0: outside it, or deposit == 0 */
	double   displacement[3];                 /* d_r, in map voxels per frame interval */
	double   distance2;                       /* d2 */
} BeamformerHipPeakPair;                      /* 48 bytes, no padding */
typedef struct {
	uint32_t frame_id[2];                     /* of frame n and frame n + 1, from their records */
	float    threshold[2];                    /* the thresholds used for them */
	uint32_t peaks[2];                        /* their stored peaks: min(found, max_per_frame) */
	uint32_t unplaced[2];                     /* stored peaks with a map coordinate that is not finite */
	uint32_t unpaired[2];                     /* placed peaks that are not in a pair of THIS frame pair */
	uint32_t first, pairs;                    /* this frame pair's records: pairs[first .. first + pairs) */
	uint32_t deposited, outside;              /* deposited + outside == pairs; both 0 when deposit == 0 */
	uint64_t found[2];                        /* exactly beamformer_hip_find_peaks_last_frames' numbers */
} BeamformerHipPeakPairs;                     /* 72 bytes, no padding */
/* The peaks of the `count` newest frames (2 <= count <= BEAMFORMER_HIP_MAX_SCORED_FRAMES), oldest first, linked frame to frame: count - 1
 * frame pairs.  region, thresholds, threshold_count and max_per_frame are beamformer_hip_find_peaks_last_frames'; the frames may differ
 * in grid and in data kind, which is why every frame may have its own placement (beamformer_hip_map_placement makes one).  rows
 * [count - 1]: a row a frame pair.  pairs (may be NULL: no record comes back, the rows and the deposits are the same) has room for
 * (count - 1) * max_per_frame records and comes back PACKED: frame pair n's records start at rows[n].first, *pair_count is their total.
 * The call runs on the library's current stream behind the frames it reads, in THREE synchronises at the most: the rows and the
 * placements go up, the mark pass and the scan run (csrc/frame_peaks.hip) and the per-frame counts come back (first synchronise); the
 * buffers are grown to what was found; the emit pass, then csrc/frame_tracks.hip: place, nearest -- the hot kernel --, match, scan and
 * emit, and the per-frame-pair numbers come back (second); exactly the pair records come back (third; skipped when pairs is NULL or
 * there is no pair; frames without a peak skip the second too).  device_ms, when not NULL: the time between events around the launches,
 * both parts added.
 * Refusals, all decided before anything is enqueued or changed and leaving every output unwritten: count < 2 or >
 * BEAMFORMER_HIP_MAX_SCORED_FRAMES, max_per_frame == 0 or > BEAMFORMER_HIP_MAX_PEAKS_PER_FRAME: BufferOverflow; InvalidAccess: rows,
 * pair_count, thresholds or placements NULL; threshold_count or placement_count neither 1 nor count; a threshold that is negative or not
 * finite; a placement entry that is not finite; max_distance not finite, negative or above BEAMFORMER_HIP_MAX_PAIR_DISTANCE;
 * deposit != 0 without a track map; and everything beamformer_hip_score_last_frames refuses -- no device in use yet, fewer than count
 * frames queued, a tombstone, an overwritten record, reused storage, a region that does not fit inside every frame, several devices. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_pair_peaks_last_frames(uint32_t count, const BeamformerHipFrameRegion *region,
                                                                     const float *thresholds, uint32_t threshold_count,
                                                                     const double *placements /* [placement_count][12] */,
                                                                     uint32_t placement_count /* 1 or count */, uint32_t use_offsets,
                                                                     float max_distance, uint32_t max_per_frame, uint32_t deposit,
                                                                     BeamformerHipPeakPairs *rows /* [count - 1] */,
                                                                     BeamformerHipPeakPair *pairs /* may be NULL; room for (count - 1) * max_per_frame */,
                                                                     uint32_t *pair_count, float *device_ms);
typedef struct {
	uint32_t points[3];
	uint32_t calls;                           /* successful beamformer_hip_pair_peaks_last_frames calls with deposit != 0, and beamformer_hip_track_peaks_last_frames or beamformer_hip_draw_tracks_last_frames calls with BEAMFORMER_HIP_TRACK_DEPOSIT_LINKS, since the reset */
	uint64_t pairs, deposited, outside;       /* their totals: pairs == deposited + outside */
} BeamformerHipTrackMapInfo;                  /* 40 bytes, no padding */
/* The track map as it is, behind everything enqueued on the current stream (one synchronise): counts[out_count] and sums[3 * voxels]
 * -- component r of voxel i at sums[r * voxels + i], voxels the map's own number, NOT out_count --; *info (may be NULL): the grid and
 * the totals since the reset.  Errors as beamformer_hip_localisation_map_copy: counts or sums NULL, no map, no device, several devices:
 * InvalidAccess; out_count below the map's voxel count: ExportSpaceOverflow. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_track_map_copy(uint32_t *counts, int64_t *sums, uint64_t out_count, BeamformerHipTrackMapInfo *info);
/* Queues ONE Float32 frame of the track map's grid into the frame ring; the map itself is left unchanged.  With n a voxel's count and
 * k = max(1, min_pairs): a voxel with n < k is 0.  Otherwise components 0..2 are the mean displacement along map axis r per frame
 * interval, (float)(((double)sum_r / 1048576.0) / (double)n) * scale -- a double division, a double division, one conversion rounded to
 * nearest, one float32 multiply --; component 3 is (float)n * scale; component 4 is the squared mean speed,
 * (float)((mx * mx + my * my) + mz * mz) * scale with the three means in double: no square root takes part, so the frame is
 * reproducible bit for bit.  The frame is placed, numbered, recorded and timed exactly as beamformer_hip_queue_localisation_map does
 * its frame, the record of the newest multi-frame push and *frame_id (may be NULL) included; its record carries image_plane_tag and the
 * parameter block of the newest frame of the most recent successful pair call with deposit.  One launch (csrc/frame_tracks.hip) on the
 * current stream; the call does not synchronise unless device_ms is not NULL.
 * Refusals, all decided before anything changes: component >= BEAMFORMER_HIP_TRACK_MAP_COMPONENTS, a scale that is not finite, no map,
 * no device, several devices, no successful pair call with deposit since the reset: InvalidAccess; a frame of the map's size that does
 * not fit the ring: FrameSizeOverflow. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_queue_track_map(uint32_t component, float scale, uint32_t min_pairs, uint32_t image_plane_tag,
                                                              uint32_t *frame_id, float *device_ms);

/* ---- peak tracks: the pairs of a call's frames chained ON THE DEVICE, and kept by length (what decides the quality of a published ULM
 * image: a detection counts only when it persists over L consecutive frames, L about 10 to 15 -- the pair call alone is L = 2 --;
 * instead of downloading every packed pair list and chaining on the host, every ensemble) ----
 * DEFINITION (tests/track_chains_ref.py restates it in numpy, on top of tests/tracks_ref.py).  All of it beyond the pairs is integer.
 * PEAKS, RANK, POSITION, DISTANCE, CHOICE and PAIR are beamformer_hip_pair_peaks_last_frames', byte for byte: the same mark, scan, emit,
 * place and nearest launches run.
 * LINK.  A pair (a, b) of frame pair n links peak a of frame n to peak b of frame n + 1: a peak has at most one link to the older frame
 * and at most one to the newer.  An UNPLACED peak has no links and belongs to no track: it counts in `unplaced` only.
 * TRACK.  A HEAD is a placed peak with no link to the older frame (every placed peak of frame 0 is one).  A track is a head followed by
 * its links toward newer frames until a peak has no link to the newer frame, the TAIL: every placed peak lies in exactly one track, of
 * L = 1 .. count peaks, one a frame, in consecutive frames.  There is NO GAP CLOSING: a frame without a partner ends the track, and what
 * follows it is another track.
 * KEPT when L >= min_length.
 * ORDER.  The kept tracks are listed in ascending (start frame, rank of the head); a track's points follow one another, oldest first,
 * and the tracks' point runs are packed in track order.  Both lists depend on the frames, the box, the thresholds, the placements,
 * max_distance, max_per_frame and min_length only: not on the call being repeated (no atomic decides a place).
 * DEPOSIT.  BEAMFORMER_HIP_TRACK_DEPOSIT_POINTS: every point of every kept track goes to the bin floor(m_r + 0.5) of the LOCALISATION
 * map -- its BIN rule --: inside the map the bin's count goes up by 1, otherwise the point counts in points_outside.
 * BEAMFORMER_HIP_TRACK_DEPOSIT_LINKS: every link of every kept track goes into the TRACK map by the pair call's DEPOSIT rule,
 * expression for expression (the midpoint, the fixed-point displacement).  Integer atomics only.
 * EQUALITIES.  (i) min_length <= 2 with LINKS leaves the track map's bytes as the pair call with deposit leaves them on the same frames
 * (every pair lies in a track of at least two peaks).  (ii) min_length == 1 with POINTS, no frame with found > max_per_frame and no
 * unplaced peak: the localisation map's bytes are beamformer_hip_accumulate_peaks_last_frames'.  (iii) The links of all tracks at
 * min_length == 1 are exactly the pair call's records. */
#define BEAMFORMER_HIP_TRACK_DEPOSIT_POINTS 1u   /* kept tracks' peaks -> the localisation map */
#define BEAMFORMER_HIP_TRACK_DEPOSIT_LINKS  2u   /* kept tracks' pairs -> the track map        */
typedef struct {
	uint32_t frame;                           /* s: the frame of the call (0 = oldest) the track begins in */
	uint32_t rank;                            /* the head's rank in frame s's find_peaks list */
	uint32_t length;                          /* L: its peaks, one a frame, in frames s .. s + L - 1 */
	uint32_t first;                           /* its points: points[first .. first + L) */
	uint32_t flags;                           /* bit 0: begins in the call's oldest frame; bit 1: ends in its newest (either may be cut by the call's window) */
	uint32_t reserved;                        /* 0 */
	double   displacement[3];                 /* m(tail) - m(head), one subtraction a row */
} BeamformerHipPeakTrack;                     /* 48 bytes, no padding */
typedef struct {
	uint32_t track;                           /* index into `tracks` */
	uint32_t frame, rank;                     /* the peak: frame of the call, rank in that frame's list */
	uint32_t deposited;                       /* bit 0: this point went into the localisation map; bit 1: its link to the next point went into the track map */
	double   position[3];                     /* m_r, the map coordinate */
} BeamformerHipTrackPoint;                    /* 40 bytes, no padding */
typedef struct {                              /* a row a FRAME */
	uint32_t frame_id; float threshold;       /* from the frame's record; the threshold used for it */
	uint32_t peaks, unplaced;                 /* stored records; those whose coordinate is not finite */
	uint32_t heads, kept_heads;               /* tracks that begin here: all of them, and those kept */
	uint32_t kept_points, kept_links;         /* this frame's peaks in kept tracks; of them, those with a link to the next frame */
	uint32_t points_deposited, points_outside, links_deposited, links_outside;   /* all 0 without the deposit bit; else the two of a kind add up to kept_points, kept_links */
	uint64_t found;                           /* exactly beamformer_hip_find_peaks_last_frames' number */
} BeamformerHipTrackedFrame;                  /* 56 bytes, no padding */
/* The peaks of the `count` newest frames (2 <= count <= BEAMFORMER_HIP_MAX_SCORED_FRAMES), oldest first, chained into tracks; every
 * argument up to max_per_frame is beamformer_hip_pair_peaks_last_frames'.  min_length: 1 .. BEAMFORMER_HIP_MAX_SCORED_FRAMES
 * (min_length > count is legal and keeps nothing).  deposit: 0 or any of the two bits.  rows[count]: a row a frame.  tracks and points
 * (either may be NULL: those records do not come back, everything else is the same) each have room for count * max_per_frame records
 * -- the convention of find_peaks' `peaks` -- and come back packed in ORDER; *track_count and *point_count are the totals (also with
 * NULL lists).  The call runs on the current stream in THREE synchronises at the most, as the pair call and for its reasons: the counts
 * (the buffers are sized by them), the per-frame tallies (the two downloads are sized by them), the records (skipped when both lists
 * are NULL or empty).  Behind the nearest kernel (csrc/frame_tracks.hip): link, ceil(log2(count)) pointer-jumping rounds, keep, the
 * scan twice, finish.  device_ms, when not NULL: the time between events around the launches, both parts added.
 * A successful call with POINTS is a depositing call of the localisation map (its calls, deposited and outside go up, the parameter
 * block of the call's newest frame is remembered for beamformer_hip_queue_localisation_map); one with LINKS is one of the track map
 * (calls, pairs -- by the kept links --, deposited, outside; beamformer_hip_queue_track_map).
 * Refusals, all decided before anything is enqueued or changed and leaving every output unwritten: everything
 * beamformer_hip_pair_peaks_last_frames refuses, with its error kinds (count < 2 among them); min_length == 0 or >
 * BEAMFORMER_HIP_MAX_SCORED_FRAMES: BufferOverflow; InvalidAccess: a deposit bit other than the two; POINTS without a localisation map,
 * LINKS without a track map; rows, track_count or point_count NULL. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_track_peaks_last_frames(uint32_t count, const BeamformerHipFrameRegion *region,
                                                                      const float *thresholds, uint32_t threshold_count,
                                                                      const double *placements /* [placement_count][12] */,
                                                                      uint32_t placement_count /* 1 or count */, uint32_t use_offsets,
                                                                      float max_distance, uint32_t max_per_frame, uint32_t min_length, uint32_t deposit,
                                                                      BeamformerHipTrackedFrame *rows /* [count] */,
                                                                      BeamformerHipPeakTrack *tracks /* may be NULL; room for count * max_per_frame */,
                                                                      BeamformerHipTrackPoint *points /* may be NULL; room for count * max_per_frame */,
                                                                      uint32_t *track_count, uint32_t *point_count, float *device_ms);

/* ---- drawn tracks: the kept tracks RASTERISED into both maps on the device.  Both maps are several times finer than the frames: a
 * bubble that moves one frame voxel a frame leaves, through the track call's DEPOSIT, one bin every 5 to 10 map cells -- a dotted
 * vessel, a velocity map with holes.  Every published ULM pipeline interpolates a kept track at map resolution before it accumulates
 * it, usually behind a short moving average along the track; this call does both where the kept tracks' points already lie, instead
 * of both record lists being downloaded and drawn on the host, every ensemble ----
 * DEFINITION (tests/track_draw_ref.py restates it in numpy, on top of tests/track_chains_ref.py).  Everything is double or integer
 * arithmetic in a fixed order, no fused multiply-add.
 * TRACKS, KEPT, ORDER are beamformer_hip_track_peaks_last_frames', byte for byte: the same launches run.  A kept track of ONE point has
 * no link and draws nothing: it counts in `lone`.
 * SMOOTH, half-width w.  Point i of a kept track with the points m_0 .. m_{L-1} (map coordinates) has the window j0 = max(0, i - w) ..
 * j1 = min(L - 1, i + w) -- clipped at the TRACK's own ends -- and s_i = (((m_j0 + m_{j0+1}) + ...) + m_j1) / (double)(j1 - j0 + 1) a
 * row: the sum in ascending j, one addition at a time, then one division.  w = 0: s_i = m_i, bit for bit.
 * LINK, EXTENT.  Link i joins s_i to s_{i+1}: d_r = s_{i+1,r} - s_{i,r}, e = max_r |d_r|.  A link with !(e <= 4096.0)
 * (BEAMFORMER_HIP_MAX_LINK_SAMPLES; a sum that overflowed to something not finite is such a link) is SKIPPED: it draws nothing, counts
 * in links_skipped, and is no predecessor.  Otherwise S = max(1, (uint32)ceil(e)).
 * SAMPLE k of 0 .. S - 1: t = ((double)k + 0.5) / (double)S, c_r = s_{i,r} + d_r * t (one multiply, then one add), B_r = floor(c_r +
 * 0.5), kept as a double.  c steps by |d_r| / S <= 1 a sample, so successive samples step by at most one cell an axis -- except on the
 * axis of a WHOLE-NUMBERED extent, where the step is 1 exactly, every c_r lies on a cell border and the rounding of t decides its side:
 * there a step may be 0 or 2.  B is monotone an axis within a link: a link never returns to a bin it has left.
 * REPEAT.  A sample's predecessor is the sample before it on the same track: sample k - 1 of its link for k > 0; for k = 0 and i > 0
 * the LAST sample of link i - 1, unless that link was skipped; otherwise it has none.  A sample whose B equals its predecessor's on all
 * three axes (compared as doubles, inside a map or not) is a REPEAT and is dropped; every other sample is DRAWN.
 * DEPOSIT.  BEAMFORMER_HIP_TRACK_DEPOSIT_POINTS: a drawn sample whose B lies inside the localisation map adds 1 there, otherwise it
 * counts in points_outside.  BEAMFORMER_HIP_TRACK_DEPOSIT_LINKS: inside the track map it adds 1 to the count and q_r = (int64)floor(d_r *
 * 1048576.0 + 0.5) to the three sums -- the pair call's fixed point, of the smoothed link; every sample of a link carries the link's own
 * d --, otherwise it counts in links_outside.  Integer atomics only: the maps' bytes stay a function of the multiset of deposits.
 * EQUALITY.  use_offsets 0, an integer placement, smooth 0 and LINKS, on frames whose links all have e <= 1 and whose rows report no
 * repeat: S = 1 and t = 0.5, the one sample is the midpoint exactly, and the track map's bytes are the track call's with LINKS. */
#define BEAMFORMER_HIP_MAX_TRACK_SMOOTH 8u          /* w, the moving average's half-width */
#define BEAMFORMER_HIP_MAX_LINK_SAMPLES 4096.0      /* a link's extent in map cells, and so its samples */
typedef struct {                              /* a row a FRAME; a link belongs to the frame of its OLDER point */
	uint32_t frame_id; float threshold;       /* from the frame's record; the threshold used for it */
	uint32_t peaks, unplaced;                 /* stored records; those whose coordinate is not finite */
	uint32_t kept_points, kept_links;         /* the track call's: this frame's peaks in kept tracks; of them, those with a link to the next frame */
	uint32_t lone;                            /* kept tracks of one point that begin (and end) here */
	uint32_t links_skipped;                   /* of kept_links, those whose extent is above the limit or not a number */
	uint32_t samples, repeats;                /* the sum of S over the other links; of them, the samples dropped as repeats */
	uint32_t points_deposited, points_outside, links_deposited, links_outside;   /* all 0 without the deposit bit; else the two of a kind add up to samples - repeats */
	uint64_t found;                           /* exactly beamformer_hip_find_peaks_last_frames' number */
} BeamformerHipDrawnFrame;                    /* 64 bytes, no padding */
#ifdef __cplusplus
static_assert(sizeof(BeamformerHipDrawnFrame) == 64, "BeamformerHipDrawnFrame: 14 words and found, no padding");
#else
_Static_assert(sizeof(BeamformerHipDrawnFrame) == 64, "BeamformerHipDrawnFrame: 14 words and found, no padding");
#endif
/* The kept tracks of the `count` newest frames drawn into the maps `deposit` names; every argument up to min_length is
 * beamformer_hip_track_peaks_last_frames'.  smooth: 0 .. BEAMFORMER_HIP_MAX_TRACK_SMOOTH.  deposit: 0 (everything is counted, nothing
 * deposited) or any of the two bits.  rows[count]: a row a frame.  No record list comes back: both live on the device for this call.
 * The call runs on the current stream in TWO synchronises: the counts (the buffers are sized by them) and the tallies.  Behind the
 * track call's launches, which deposit nothing here (csrc/frame_tracks.hip): smooth (not for smooth == 0), draw.  device_ms, when not
 * NULL: the time between events around the launches, both parts added.
 * A successful call with POINTS is a depositing call of the localisation map (calls, deposited, outside, the remembered parameter
 * block); one with LINKS is one of the track map, whose `pairs` goes up by the drawn samples, so that pairs == deposited + outside
 * still holds.  beamformer_hip_queue_localisation_map and beamformer_hip_queue_track_map work on the drawn maps unchanged.
 * Refusals, all decided before anything is enqueued or changed and leaving every output unwritten: everything
 * beamformer_hip_track_peaks_last_frames refuses, with its error kinds; smooth > BEAMFORMER_HIP_MAX_TRACK_SMOOTH: BufferOverflow;
 * InvalidAccess: a deposit bit other than the two, a bit without its map, rows NULL. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_draw_tracks_last_frames(uint32_t count, const BeamformerHipFrameRegion *region,
                                                                      const float *thresholds, uint32_t threshold_count,
                                                                      const double *placements /* [placement_count][12] */,
                                                                      uint32_t placement_count /* 1 or count */, uint32_t use_offsets,
                                                                      float max_distance, uint32_t max_per_frame, uint32_t min_length,
                                                                      uint32_t smooth, uint32_t deposit,
                                                                      BeamformerHipDrawnFrame *rows /* [count] */, float *device_ms);

/* ---- ensemble filter: a linear slow-time operator on the frames of the frame ring (the clutter filter between "ensemble" and "peaks"
 * of the ULM loop: tissue lies 30 - 60 dB above the microbubbles, so the peaks of an unfiltered ensemble are tissue speckle).  Two
 * device primitives and one host helper: the K x K slow-time Gram matrix of the K newest frames, reduced where they lie; a projector
 * made from it on the host; and a mix that writes M linear combinations of the K frames back INTO THE RING as ordinary frames, so that
 * beamformer_hip_find_peaks_last_frames, beamformer_hip_score_last_frames, beamformer_hip_copy_frame, beamformer_hip_get_frame_info and
 * beamformer_get_last_frames work on them unchanged.  The weights are the caller's: SVD clutter filtering (the projector below),
 * polynomial-regression and FIR wall filters, weighted compounding and frame differencing are all one mix ----
 * DEFINITIONS (tests/ensemble_ref.py restates them in numpy).
 * GRAM.  The K frames have one grid and one data kind.  G[j][k] = sum over v of conj(f_j[v]) * f_k[v], over the voxels v of the box
 * that are finite in EVERY one of the K frames (a voxel is finite when both its floats are); a voxel that is not finite in some frame
 * counts in non_finite and in no entry, so G stays a Gram matrix: Hermitian, positive semidefinite.  Each float is widened to double;
 * the real part of a term is rj * rk + ij * ik and the imaginary part rj * ik - ij * rk -- the products are exact in double, each part
 * is one double addition --; the voxel sum is a double sum in an order the box and K alone fix (no atomics): the bytes of `gram` depend
 * on the K frames and the box only and repeat bit for bit.  Only j <= k is computed; G[k][j] is stored as the exact conjugate of G[j][k];
 * the imaginary part of a diagonal entry is exactly 0, and real frames give imaginary parts of exactly 0 everywhere.  Index 0 is the
 * oldest frame, the order of beamformer_get_last_frames.
 * MIX.  The K frames, of one grid and one kind, give out_count new frames of that grid and kind.  Frames and weights are interleaved
 * floats.  For output j and voxel v each of the two output floats is ONE float32 fmaf chain from +0 in ascending k --
 *     real:       acc = fmaf(Wre[j][k], re_k, acc), then acc = fmaf(-Wim[j][k], im_k, acc)
 *     imaginary:  acc = fmaf(Wim[j][k], re_k, acc), then acc = fmaf( Wre[j][k], im_k, acc)
 * -- no weight is skipped for being zero, so a voxel that is not finite in some frame is not finite in every output (plain IEEE).  Real
 * frames use the real parts only: acc = fmaf(Wre[j][k], f_k, acc). */
#define BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES 256u
typedef struct {
	uint32_t count;                           /* K */
	uint32_t data_kind;                       /* of the frames */
	uint32_t points[3];                       /* the frames' common grid */
	uint32_t region_first[3], region_count[3];/* the box that was reduced (the whole frame when region == NULL) */
	uint32_t first_frame_id;                  /* the frames have ids first_frame_id .. first_frame_id + K - 1 */
	uint64_t voxels;                          /* voxels of the box finite in ALL K frames: what every entry sums over */
	uint64_t non_finite;                      /* voxels of the box not finite in at least one frame */
} BeamformerHipEnsembleInfo;                  /* 64 bytes, no padding */
/* gram[count][count][2] doubles (re, im), row j column k as above.  Three launches (csrc/ensemble.hip: the all-finite mask, the
 * partial pass, the fold) are enqueued on the library's current stream behind the frames they read; the matrix and the counts come
 * back through one device-to-host copy and one stream synchronise.  info may be NULL.  device_ms, when not NULL: the time between two
 * events around the launches.
 * Refusals, all decided before anything is enqueued and leaving every output unwritten: count == 0 or
 * > BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES: BufferOverflow; gram == NULL: InvalidAccess; frames that differ in grid or in data kind:
 * DataSizeMismatch; and everything beamformer_hip_score_last_frames refuses (InvalidAccess) -- no device in use yet, fewer than count
 * frames queued, a tombstone, an overwritten record, reused storage, a region that does not fit inside the frames, several devices --
 * and a box of 2^32 voxels or more. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_gram_last_frames(uint32_t count, const BeamformerHipFrameRegion *region,
                                                               double *gram, BeamformerHipEnsembleInfo *info, float *device_ms);
/* Host only: touches no device and no library state but the last error.  A cyclic Jacobi eigendecomposition, in double, of the
 * Hermitian matrix whose UPPER triangle gram[count][count][2] holds (the imaginary parts of the diagonal are not read).  With the
 * eigenpairs (lambda_i, u_i) in descending order of lambda, weights = sum over i from remove_high to count - remove_low - 1 of
 * u_i u_i^H, rounded once to float32: the projector that removes the remove_high strongest slow-time components (tissue) and the
 * remove_low weakest (noise).  It does not depend on the phases of the u_i; within a cluster of equal eigenvalues it is defined only
 * when the cut does not split the cluster.  remove_high + remove_low == count gives zeros, 0 and 0 the identity up to rounding.
 * weights[count][count][2] floats; eigenvalues[count], descending, may be NULL.  InvalidAccess: gram or weights NULL, remove_high +
 * remove_low > count, an entry of the upper triangle that is not finite; count == 0 or > BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES:
 * BufferOverflow. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_clutter_projector(const double *gram, uint32_t count, uint32_t remove_high, uint32_t remove_low,
                                                                float *weights, double *eigenvalues);
/* weights[out_count][count][2] floats; index 0 of the second dimension is the oldest source frame.  The out_count outputs are placed
 * in the frame ring as ONE contiguous run by the rule every push follows (a run that would straddle the end starts again at offset 0;
 * the records whose storage it reuses stop being exportable), with consecutive ids from the counters a push advances; their records
 * carry the newest source frame's parameter block and the call's image_plane_tag; their rows of the timing table report no stages and 0 DAS
 * voxels.  *first_frame_id (may be NULL): the oldest output's id.  The record of the newest multi-frame push is left alone --
 * beamformer_hip_get_last_burst_info and its kin go on describing that push behind the outputs -- until an output takes the timing
 * slot (one of 32, by id) that holds the push's events; from then on those calls fail as they do after any other push.
 * One launch (csrc/ensemble.hip), enqueued on the current stream behind the frames it reads; the weights travel through pinned memory
 * of the call's own.  The call does not synchronise unless device_ms is not NULL (then: the time between two events around the launch).
 * Refusals, all decided BEFORE ANYTHING CHANGES -- the counters, the records, the ring's next offset -- and leaving every output
 * unwritten: count or out_count 0 or > BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES: BufferOverflow; weights == NULL, a weight that is not
 * finite, a nonzero imaginary weight on real frames: InvalidAccess; frames that differ in grid or kind: DataSizeMismatch; a run of
 * out_count frames that does not fit the ring, or that -- placed by the rule above -- would reuse storage of one of its own count
 * source frames: FrameSizeOverflow; and everything beamformer_hip_score_last_frames refuses (InvalidAccess). */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_mix_last_frames(uint32_t count, const float *weights, uint32_t out_count,
                                                              uint32_t image_plane_tag, uint32_t *first_frame_id, float *device_ms);

/* ---- block-wise ensemble filter: the filter above made local.  Over a real field of view the slow-time statistics are not uniform --
 * tissue moves differently from region to region, the noise floor rises with depth --, and one SVD cut for the whole frame leaves tissue
 * in one part of the image and eats bubbles in another.  The block-wise filter takes a Gram matrix and a projector for each of many
 * overlapping boxes and blends the filtered blocks by a window: here the Gram matrices of all boxes in ONE call, a host helper that lays
 * the boxes on a lattice of nodes, and a mix whose weight table is given at those nodes and interpolated between them, as
 * beamformer_hip_warp_last_frames interpolates its displacement field -- the pair that beamformer_hip_correlate_last_frames and the warp
 * are for motion.  Out of scope: an autocorrelation that takes a weight field, any rule that picks the rank of a box ----
 * Axis a: 0 = x (the fastest), 1 = y, 2 = z.  Index 0 is the oldest frame.  tests/block_filter_ref.py restates the definitions in numpy.
 *
 * beamformer_hip_gram_boxes_last_frames.
 * DEFINITION.  The matrix and the info of box b are byte for byte what beamformer_hip_gram_last_frames(count, &regions[b], ...) returns on
 * the same frames, `voxels` and `non_finite` included: the partition of a box into chunks is that call's, a function of the box and
 * count alone.  The result of a box does not depend on the other boxes, their order, their overlap, or on the call being repeated; boxes
 * may overlap, repeat and differ in size.
 * OUTPUTS.  grams[region][count][count][2] doubles; infos[region], may be NULL.  device_ms, when not NULL: the time between two events
 * around the launches.
 * The boxes are walked in batches whose partial sums (16 KiB a chunk and tile pair) fit a budget of 64 MiB; a batch is three launches
 * (csrc/ensemble_blocks.hip: the passes of the single-box call, each over all boxes of the batch), the batches lie behind one another on
 * the library's current stream behind the frames they read.  A call costs ONE upload, ONE device-to-host copy and ONE stream
 * synchronise, however many boxes.
 * Refusals, all decided before anything is enqueued and leaving every output unwritten: count == 0 or
 * > BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES, region_count == 0 or > BEAMFORMER_HIP_MAX_GRAM_BOXES, region_count x count x count >
 * BEAMFORMER_HIP_MAX_GRAM_BOX_ENTRIES: BufferOverflow (decided first); grams or regions NULL, a box with a zero count or one that does
 * not fit inside the frames, a box of 2^32 voxels or more, and everything beamformer_hip_gram_last_frames refuses, several devices
 * included: InvalidAccess; frames that differ in grid or in data kind: DataSizeMismatch. */
#define BEAMFORMER_HIP_MAX_GRAM_BOXES        1024u
#define BEAMFORMER_HIP_MAX_GRAM_BOX_ENTRIES  (1u << 22)   /* region_count x count x count: a result of at most 64 MiB */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_gram_boxes_last_frames(uint32_t count, const BeamformerHipFrameRegion *regions, uint32_t region_count,
                                                                     double *grams /* [region][count][count][2] */,
                                                                     BeamformerHipEnsembleInfo *infos /* [region], may be NULL */,
                                                                     float *device_ms);
/* Host only: touches no device and no library state but the last error.  The boxes of a lattice of N_a = nodes[a] nodes an axis on a
 * grid of `points`.  Node j of axis a sits at voxel P_j = node_first[a] + j * node_step[a], computed in 64 bits: a node may lie beyond
 * the frame.  Its box along that axis is [max(0, P_j - half[a]), min(points[a], P_j + half[a] + 1)); the box of node (jx, jy, jz) is the
 * product of its three, written to regions[(jz * Ny + jy) * Nx + jx] -- the flat node order of the weight table of
 * beamformer_hip_mix_field_last_frames.  node_step[a] is not read where N_a == 1.
 * Refusals, leaving regions unwritten: a NULL pointer, a points or nodes entry of 0, node_step[a] == 0 with N_a > 1, a box that misses
 * the frame (no voxel along some axis): InvalidAccess; the product of nodes > BEAMFORMER_HIP_MAX_MIX_NODES: BufferOverflow. */
#define BEAMFORMER_HIP_MAX_MIX_NODES         1024u        /* product of nodes */
#define BEAMFORMER_HIP_MAX_MIX_FIELD_ENTRIES (1u << 22)   /* product of nodes x out_count x count */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_lattice_boxes(const uint32_t points[3], const uint32_t nodes[3], const uint32_t node_first[3],
                                                            const uint32_t node_step[3], const uint32_t half[3],
                                                            BeamformerHipFrameRegion *regions /* [product of nodes], node order */);
/* beamformer_hip_mix_field_last_frames: a mix whose weight table varies over the frame.
 * DEFINITION.
 * SOURCES.  The `count` = K newest frames of the ring, of one grid and one kind: beamformer_hip_mix_last_frames' rules.
 * CORNER VALUES.  weights[node][out_count][count][2] floats, the nodes in the flat order above.  For node c, output j and voxel v,
 * y_c[j][v] is the MIX chain above under W[c][j][.] -- the same order, the same signs, no weight skipped --: bit for bit what
 * beamformer_hip_mix_last_frames would store for that table.
 * SEGMENTS.  Along axis a with N = nodes[a], for a voxel of index i: N == 1: node 0, no interpolation (node_first[a] and node_step[a]
 * are not read); i < P_0: node 0 alone; i >= P_(N-1): node N - 1 alone; otherwise j = (i - node_first[a]) / node_step[a],
 * r = (i - node_first[a]) - j * node_step[a] and t = (float)r * inv, inv = 1.0f / (float)node_step[a] (one float32 division, on the
 * host): nodes j and j + 1 are blended.
 * BLEND.  Each output float is blended by lerps fmaf(t, b - a, a), a the value at the lower node: along x -- for each of the up to four
 * (y, z) corner choices --, then along y over those results, then along z.  An axis on which the voxel has a single node contributes
 * that node's value and no lerp.  Plain IEEE otherwise: a source voxel that is not finite makes every output at it not finite (NaN
 * payloads are not promised).
 * So nodes = {1, 1, 1} gives beamformer_hip_mix_last_frames' bytes; equal tables at all nodes give them wherever the outputs are
 * finite; a voxel outside the lattice on every interpolated axis has the plain mix's bytes under that corner node.  The bytes of output
 * j depend on the sources, the rows W[.][j][.] and the lattice only -- not on out_count, on the other rows, or on repetition.
 * OUTPUTS.  out_count new frames of the sources' grid and kind in ONE contiguous run, placed, numbered, recorded and timed exactly as
 * beamformer_hip_mix_last_frames' run is, the record of the newest multi-frame push and *first_frame_id (may be NULL) included.
 * One launch (csrc/ensemble_blocks.hip), enqueued on the current stream behind the frames it reads; the weights travel through pinned
 * memory of the call's own.  The call does not synchronise unless device_ms is not NULL (then: the time between two events around the
 * launch).
 * Refusals, all decided BEFORE ANYTHING CHANGES and leaving every output unwritten: count or out_count 0 or
 * > BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES: BufferOverflow (decided first); weights, nodes, node_first or node_step NULL: InvalidAccess;
 * a nodes entry of 0, the product of nodes > BEAMFORMER_HIP_MAX_MIX_NODES, that product x out_count x count >
 * BEAMFORMER_HIP_MAX_MIX_FIELD_ENTRIES: BufferOverflow; node_step[a] == 0 with N_a > 1, a weight that is not finite, a nonzero imaginary
 * weight on real frames, a frame of more than 2^31 - 1 voxels, and everything beamformer_hip_score_last_frames refuses, several devices
 * included: InvalidAccess; frames that differ in grid or kind: DataSizeMismatch; a run of out_count frames that does not fit the ring,
 * or that would reuse storage of one of its own count source frames: FrameSizeOverflow. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_mix_field_last_frames(uint32_t count, const float *weights /* [node][out_count][count][2] */,
                                                                    const uint32_t nodes[3], const uint32_t node_first[3],
                                                                    const uint32_t node_step[3], uint32_t out_count, uint32_t image_plane_tag,
                                                                    uint32_t *first_frame_id, float *device_ms);

/* ---- slow-time autocorrelation of an ensemble: the per-voxel reduction ACROSS the frames, behind the filter above.  Lag 0 is the power
 * Doppler image of the filtered ensemble, lag 1 the Kasai estimate (its angle is the axial velocity: v = angle(R_1) c PRF / (4 pi f0),
 * the angle is the caller's), lags 0 and 1 together the variance.  The filter is whatever weight table the caller would hand to
 * beamformer_hip_mix_last_frames, under the same definition; the filtered frames are never stored ----
 * DEFINITION (tests/autocorr_ref.py restates it in numpy).
 * SOURCES.  The `count` = K newest frames of the ring, of one grid and one kind: beamformer_hip_mix_last_frames' rules.  Index 0 is the
 * oldest frame.
 * FILTERED SAMPLES.  weights[rows][count][2] floats.  y_n[v] = sum over k of W[n][k] f_k[v], n = 0 .. rows - 1: each float is exactly the
 * float32 fmaf chain of MIX above -- the same order, the same signs, no weight skipped --, so y_n is bit for bit what
 * beamformer_hip_mix_last_frames would have stored.  weights == NULL is the identity: y_n = f_n, and rows must equal count (an ensemble
 * that is filtered already, or no filter at all).
 * LAG PRODUCTS.  For L = 0 .. lag_count - 1: R_L[v] = sum over n = 0 .. rows - 1 - L of conj(y_n[v]) y_{n+L}[v].  Each output float is
 * ONE float32 fmaf chain from +0 in ascending n --
 *     real:       acc = fmaf(yr_n, yr_{n+L}, acc), then acc = fmaf( yi_n, yi_{n+L}, acc)
 *     imaginary:  acc = fmaf(yr_n, yi_{n+L}, acc), then acc = fmaf(-yi_n, yr_{n+L}, acc)
 * -- but the imaginary part of lag 0, which is no chain (it would leave rounding residue): it is stored as 0 * re(R_0), exactly +0
 * where that real part is finite and NaN where it is not.  Real frames run acc = fmaf(y_n, y_{n+L}, acc) only.  Plain IEEE otherwise:
 * a voxel that is not finite in some source frame is not finite in every output float.
 * OUTPUTS.  lag_count new frames of the sources' grid and kind, lag 0 first, placed in the ring as ONE contiguous run exactly as
 * beamformer_hip_mix_last_frames places its run: the same ids from the counters a push advances, the newest source's parameter block,
 * the call's image_plane_tag, rows of the timing table that report no stages and 0 DAS voxels, the same treatment of the record of the
 * newest multi-frame push.  beamformer_hip_find_peaks_last_frames, beamformer_hip_score_last_frames, beamformer_hip_copy_frame,
 * beamformer_hip_get_frame_info and beamformer_get_last_frames work on them unchanged.  *first_frame_id (may be NULL): the id of lag 0.
 * One launch (csrc/autocorr.hip), enqueued on the current stream behind the frames it reads; the call does not synchronise unless
 * device_ms is not NULL (then: the time between two events around the launch).
 * Refusals, all decided BEFORE ANYTHING CHANGES and leaving every output unwritten: count or rows 0 or
 * > BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES: BufferOverflow; lag_count 0, > BEAMFORMER_HIP_MAX_LAGS or > rows, weights == NULL with
 * rows != count, a weight that is not finite, a nonzero imaginary weight on real frames: InvalidAccess; frames that differ in grid or
 * kind: DataSizeMismatch; a run of lag_count frames that does not fit the ring, or that would reuse storage of one of its own count
 * source frames: FrameSizeOverflow; and everything beamformer_hip_score_last_frames refuses (InvalidAccess). */
#define BEAMFORMER_HIP_MAX_LAGS 4u
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_autocorrelate_last_frames(uint32_t count, const float *weights, uint32_t rows,
                                                                        uint32_t lag_count, uint32_t image_plane_tag,
                                                                        uint32_t *first_frame_id, float *device_ms);

/* ---- spatial filter: a separable convolution of ring frames, written back into the ring.  The operators above work across the
 * ensemble, voxel by voxel, or reduce a frame to numbers; this one takes frames and gives spatially filtered frames: the PSF-sized
 * Gaussian in front of beamformer_hip_find_peaks_last_frames (without it the maxima are those of the speckle), the box average of the
 * lag frames of beamformer_hip_autocorrelate_last_frames in front of the Kasai angle, and -- normalised -- a smoothing that neither
 * darkens a frame at its edges nor spreads the NaN of a coherency-weighted frame, and fills the holes ----
 * DEFINITION (tests/spatial_ref.py restates it in numpy).
 * SOURCES.  The `count` newest frames of the ring, of one grid and one kind: beamformer_hip_mix_last_frames' rules.
 * TAPS.  Axis a (0 = x, the fastest; 1 = y; 2 = z) has n = tap_counts[a] real taps h = taps[a][0 .. n - 1]; n is odd and
 * <= BEAMFORMER_HIP_MAX_SPATIAL_TAPS, its radius r = (n - 1) / 2.  n == 0 (taps[a] is then not read and may be NULL) leaves the axis
 * alone: no pass, no rounding.  Real taps act on the real and the imaginary float of a complex voxel independently.
 * A PASS along axis a turns a field f into g; each float of g is ONE float32 fmaf chain from +0 in ascending t,
 *     acc = fmaf(h[t], f[i + r - t], acc),   t = 0 .. n - 1,
 * i the voxel's index along the axis -- a true convolution: taps {0, 0, 1} move the frame by +1 voxel --, and a term whose source index
 * i + r - t lies outside the frame is skipped.  The passes run in the order x, y, z over the axes with n > 0; each reads the float32
 * result of the one before it.
 * mode BeamformerHipSpatialMode_Zero: plain IEEE otherwise.  No tap is skipped for being zero: a voxel that is not finite makes every
 * output whose support covers it not finite, as the mix does.
 * mode BeamformerHipSpatialMode_Normalised: m[v] = 1 where the source voxel is finite (both floats of a complex one), else 0.  The
 * numerator N is the passes above with the terms of the non-finite source voxels SKIPPED in the first pass as out-of-frame terms are;
 * the denominator D is the same passes applied to m, acc = fmaf(h[t], m[i + r - t], acc), the same terms skipped.  Each output float is
 * the IEEE float32 quotient N / D; where no finite voxel lies under a positive tap that is +0 / +0 = NaN.  A voxel that is not finite
 * but has finite neighbours under the taps gets a finite output: the hole is filled; a constant frame stays constant up to its edges.
 * Taps must be >= 0 in this mode.
 * The bytes of an output depend on its source frame, the taps and the mode only -- not on count, on the other frames of the call, or on
 * the call being repeated.
 * OUTPUTS.  `count` new frames of the sources' grid and kind, output n source n filtered, oldest first, placed in the ring as ONE
 * contiguous run exactly as beamformer_hip_mix_last_frames places its run: the same ids from the counters a push advances, the newest
 * source's parameter block, the call's image_plane_tag, rows of the timing table that report no stages and 0 DAS voxels, the same
 * treatment of the record of the newest multi-frame push.  Everything that reads frames works on them unchanged.  *first_frame_id (may
 * be NULL): the id of the oldest output.  One launch a live axis (csrc/spatial.hip), enqueued on the current stream behind the frames
 * they read; what lies between two passes is memory of the library's own and the output run itself, never another frame of the ring.
 * The call does not synchronise unless device_ms is not NULL (then: the time between two events around the launches).
 * Refusals, all decided BEFORE ANYTHING CHANGES and leaving every output unwritten: count 0 or > BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES, a
 * tap count > BEAMFORMER_HIP_MAX_SPATIAL_TAPS: BufferOverflow; taps or tap_counts NULL, an even tap count, taps[a] NULL with a nonzero
 * count, all three counts 0, a tap that is not finite, a tap < 0 in Normalised mode, an unknown mode: InvalidAccess;
 * frames that differ in grid or kind: DataSizeMismatch; a run of `count` frames that does not fit the ring, or that would reuse storage
 * of one of its own source frames: FrameSizeOverflow; and everything beamformer_hip_score_last_frames refuses, several devices
 * included (InvalidAccess).  A tap count larger than an axis's extent is legal, also on an axis of 1 point: the skipped terms handle
 * it. */
#define BEAMFORMER_HIP_MAX_SPATIAL_TAPS 33u
typedef enum {
	BeamformerHipSpatialMode_Zero       = 0,
	BeamformerHipSpatialMode_Normalised = 1,
	BeamformerHipSpatialMode_Count
} BeamformerHipSpatialMode;
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_convolve_last_frames(uint32_t count, const float *const taps[3], const uint32_t tap_counts[3],
                                                                   uint32_t mode, uint32_t image_plane_tag,
                                                                   uint32_t *first_frame_id, float *device_ms);

/* ---- shift correlation: frame-to-frame motion estimated on the device.  Every operator above assumes that voxel v of frame k and
 * voxel v of frame j show the same tissue; over an ensemble they do not.  This call correlates each of the K newest frames with one of
 * them at every integer shift of a window, over one box (rigid motion) or many small ones (block matching: a displacement field), and
 * a host helper turns the tables into displacements.  beamformer_hip_warp_last_frames (below) applies them: it resamples the frames
 * at the displaced positions, per frame or as a field ----
 * DEFINITION (tests/motion_ref.py restates it in numpy).
 * SOURCES.  The `count` = K newest frames of the ring, of one grid and one kind: beamformer_hip_gram_last_frames' rules and refusals.
 * Index 0 is the oldest frame; ref is frame `reference` (< K).
 * SHIFTS.  S_a = max_shift[a] (a: 0 = x, the fastest; 1 = y; 2 = z), a shift s = (sx, sy, sz) with |s_a| <= S_a, T = the product of
 * the (2 S_a + 1); the flat shift index is ((sz + Sz)(2 Sy + 1) + (sy + Sy))(2 Sx + 1) + (sx + Sx).
 * BOXES.  regions NULL: one box, the frame whole (region_count is not read and reported as 1); else region_count boxes, which may
 * overlap and differ in size.
 * TERMS.  For box b, frame k and shift s: the voxels v inside the box with v + s inside the FRAME (not the box: a shifted read leaves
 * the box freely, as the peaks' neighbourhoods do), ref[v] finite and f_k[v + s] finite (a complex voxel: both floats).
 * SUMS over the terms: re + i im = sum conj(ref[v]) f_k[v + s]; energy_reference = sum |ref[v]|^2; energy_frame = sum |f_k[v + s]|^2;
 * terms = their number.  The arithmetic is the Gram matrix's: every float widened to double, the products exact; the real part
 * rj rk + ij ik, the imaginary part rj ik - ij rk and a squared magnitude r r + i i are ONE rounding each (written as an fma), adding
 * one to its running sum is one more.  Real frames take i = 0: every im is exactly 0.  An entry without terms is 40 zero bytes.
 * SIGN.  If frame k is the reference moved by d voxels, f_k[v + d] = ref[v], then |C| peaks at s = d.
 * OUTPUT.  table[region][frame][shift]: K tables a region, the reference's own -- its spatial autocorrelation -- included; that one's
 * entry at s = 0 has im == 0 and re == energy_reference == energy_frame.
 * ORDER.  Every sum is a double sum in an order that the box and the window alone fix, no atomics: the 40 bytes of an entry depend on
 * the reference frame, frame k, the box and max_shift only -- not on K, on the other frames, on the other regions or their order, or
 * on the call being repeated.
 * Two launches (csrc/correlate.hip), enqueued on the current stream behind the frames they read; the table comes back through one
 * device-to-host copy and one synchronise.  info and device_ms may be NULL; device_ms: the time between two events around the launches.
 * Refusals, all decided BEFORE ANYTHING IS ENQUEUED and leaving every output unwritten: count 0 or > BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES,
 * region_count 0 (regions given) or > BEAMFORMER_HIP_MAX_CORRELATION_REGIONS, a max_shift entry > BEAMFORMER_HIP_MAX_SHIFT,
 * T > BEAMFORMER_HIP_MAX_SHIFTS, regions x K x T > BEAMFORMER_HIP_MAX_CORRELATION_ENTRIES: BufferOverflow; table or max_shift NULL,
 * reference >= count, a region with a zero count or one that does not fit inside the frames, a box of 2^32 voxels or more, and
 * everything beamformer_hip_score_last_frames refuses, several devices included: InvalidAccess; frames that differ in grid or kind:
 * DataSizeMismatch.  A window wider than an axis is legal, also on an axis of 1 point: its out-of-frame shifts have no terms. */
#define BEAMFORMER_HIP_MAX_SHIFT                16u          /* per axis */
#define BEAMFORMER_HIP_MAX_SHIFTS               1089u        /* product of (2 S_a + 1): 33 x 33 on a plane, 9 x 9 x 9 in a volume */
#define BEAMFORMER_HIP_MAX_CORRELATION_REGIONS  256u
#define BEAMFORMER_HIP_MAX_CORRELATION_ENTRIES  (1u << 20)   /* regions x frames x shifts */
typedef struct {
	double   re, im, energy_reference, energy_frame;
	uint64_t terms;
} BeamformerHipShiftCorrelation;              /* 40 bytes, no padding */
typedef struct {
	uint32_t count, reference, data_kind, region_count;
	uint32_t points[3], max_shift[3];
	uint32_t shifts;                          /* T */
	uint32_t first_frame_id, reference_frame_id;
	uint32_t reserved;
} BeamformerHipCorrelationInfo;               /* 56 bytes, no padding */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_correlate_last_frames(uint32_t count, uint32_t reference, const BeamformerHipFrameRegion *regions,
                                                                    uint32_t region_count, const uint32_t max_shift[3],
                                                                    BeamformerHipShiftCorrelation *table, BeamformerHipCorrelationInfo *info,
                                                                    float *device_ms);
/* Host only (no device, no library state but the last error): one displacement a table of T entries, in double.
 * CANDIDATES: the entries with terms > 0, all four doubles finite and -- when `normalised` -- both energies > 0.
 * SCORE q = re^2 + im^2, divided by energy_reference * energy_frame when `normalised`.  PEAK: the largest q, the lowest flat shift
 * index among equals; m = sqrt(q).  FIT: axis a is fitted when S_a > 0, both neighbours at -1 and +1 along it lie in the window and
 * are candidates, and den = (m- + m+) - (m0 + m0) < 0; then offset = 0.5 (m- - m+) / den, clamped to [-0.5, 0.5] (the peaks'
 * parabola, in double).  A table without a candidate gives a row of zero bytes.  Returns 1 when at least one table had a candidate;
 * 0 with InvalidAccess for a NULL argument, or when no table had one (out is filled all the same); 0 with BufferOverflow for
 * table_count 0, a max_shift entry > BEAMFORMER_HIP_MAX_SHIFT or T > BEAMFORMER_HIP_MAX_SHIFTS. */
typedef struct {
	float    displacement[3];                 /* voxels: integer peak + sub-voxel offset */
	int32_t  shift[3];                        /* the integer peak */
	float    coefficient;                     /* |C| / sqrt(energy_reference * energy_frame) at the peak, 0 where an energy is 0 */
	float    phase;                           /* atan2(im, re) at the peak: sub-wavelength axial motion of IQ frames */
	uint32_t fitted;                          /* bit a: axis a was fitted */
	uint32_t at_window_edge;                  /* bit a: S_a > 0 and |shift[a]| == S_a -- the true shift may lie outside the window */
} BeamformerHipDisplacement;                  /* 40 bytes, no padding */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_displacements_from_correlation(const BeamformerHipShiftCorrelation *tables, uint32_t table_count,
                                                                             const uint32_t max_shift[3], uint32_t normalised,
                                                                             BeamformerHipDisplacement *out);

/* ---- warp: ring frames resampled at displaced positions, written back into the ring: motion compensation.  The shift correlation
 * above estimates how the frames of an ensemble moved; this call applies the estimate -- a rigid shift per frame or a displacement
 * field on a lattice of nodes (the block-matching result) --, so that the slow-time operators behind it (Gram matrix, mix,
 * autocorrelation, peaks) see voxel v of every frame on the same tissue ----
 * DEFINITION (tests/warp_ref.py restates it in numpy).  Every operation named below is ONE float32 operation, fmaf one rounding.
 * SOURCES.  The `count` = K newest frames of the ring, of one grid (nx, ny, nz) and one kind: beamformer_hip_mix_last_frames' rules
 * and refusals.  Index 0 is the oldest frame.  Axis a: 0 = x, the fastest; 1 = y; 2 = z.
 * FIELD.  field[frame][jz][jy][jx][3] floats: the displacement in voxels (x, y, z) at the nodes of a lattice of N_a = nodes[a] >= 1
 * nodes an axis; node j of axis a sits at voxel coordinate node_first[a] + j * node_step[a].  One lattice for all frames, values per
 * frame; nodes = {1, 1, 1}: a rigid shift per frame.  The displacement d(v) at voxel v = (vx, vy, vz) is the trilinear interpolation
 * of the nodes, constant outside the lattice: per axis with N_a > 1
 *     c_a = ((float)v_a - node_first[a]) * inv_step_a,   inv_step_a = 1.0f / node_step[a] (one float32 division, on the host),
 *     c_a clamped to [0, N_a - 1] (fmaxf, then fminf),   j_a = min((int)floorf(c_a), N_a - 2),   s_a = c_a - (float)j_a,
 * and per component the lerps  fmaf(s, b - a, a)  (a: the value at the lower index) along x between nodes j_x and j_x + 1 -- for each
 * of the four (j_y + 0 | 1, j_z + 0 | 1) --, then along y over those results, then along z.  An axis with N_a == 1 is not interpolated:
 * its node index is 0, its lerp is left out, node_first[a] and node_step[a] are not read.
 * SIGN.  Output n at voxel v is source n sampled at p = v + d_n(v): the correlation's sign -- if f_k[v + d] = ref[v], warping f_k by d
 * gives ref --, so a BeamformerHipDisplacement.displacement goes into the field as it is.
 * POSITION AND WEIGHTS.  Per axis with more than one point: p_a = (float)v_a + d_a, i_a = floorf(p_a), t = p_a - i_a.
 * BeamformerHipWarpInterpolation_Linear: taps at i_a, i_a + 1 with weights  1.0f - t,  t.
 * BeamformerHipWarpInterpolation_Cubic: Catmull-Rom, taps at i_a - 1 .. i_a + 2 with weights
 *     w0 = fmaf(fmaf(-0.5f, t, 1.0f), t, -0.5f) * t,          w1 = fmaf(fmaf(1.5f, t, -2.5f) * t, t, 1.0f),
 *     w2 = fmaf(fmaf(-1.5f, t, 2.0f), t, 0.5f) * t,           w3 = (fmaf(0.5f, t, -0.5f) * t) * t.
 * An axis of ONE point is not interpolated: that component of the field is not read, and the axis has one tap, at index 0, of weight
 * exactly 1.0f -- a view plane costs 4 taps (Linear) or 16 (Cubic), not 8 or 64.  There is no nearest mode.
 * SUM.  Separable: along x for every (y, z) row of the support, then along y over those results, then along z; each of these is ONE
 * float32 fmaf chain from +0 in ascending tap index, acc = fmaf(w, value, acc); the real and the imaginary float of a complex voxel
 * are independent chains under the same weights.
 * EDGE.  BeamformerHipWarpEdge_Zero: a term whose source index (along the chain's axis) lies outside the frame is skipped, as the
 * convolution skips it; a chain without terms is +0.  BeamformerHipWarpEdge_Clamp: the index is clamped to 0 .. extent - 1 -- the
 * edge voxel repeats, and a compensated frame does not darken at its rim.  Both make the output a continuous function of p.
 * Otherwise plain IEEE: a source voxel under the support that is not finite makes the output not finite, no weight is skipped for
 * being zero.
 * ROTATIONS.  rotations[frame][2] = (re, im), may be NULL (then nothing is multiplied).  After the sum a complex output (x, y) becomes
 *     re' = fmaf(-im, y, fmaf(re, x, +0)),   im' = fmaf(re, y, fmaf(im, x, +0))
 * -- the mix's two chains for a one-term product: exp(-i phase) of a displacement's `phase` is the phase correction an IQ ensemble
 * needs after axial motion.  A real output x becomes fmaf(re, x, +0); a nonzero imaginary part on real frames is refused.
 * The bytes of output n depend on source n, its own rows of the field and of the rotations, the lattice and the two modes only -- not
 * on count, on the other frames, on the call being repeated, or on which of the kernel's two paths a tile took.
 * OUTPUTS.  `count` new frames of the sources' grid and kind, output n source n warped, oldest first, placed, numbered, recorded and
 * timed exactly as beamformer_hip_convolve_last_frames' run is, the record of the newest multi-frame push and *first_frame_id (may be
 * NULL) included.  One launch (csrc/warp.hip) on the current stream behind the frames it reads; the call does not synchronise unless
 * device_ms is not NULL (then: the time between two events around the launch).
 * Refusals, all decided BEFORE ANYTHING CHANGES and leaving every output unwritten: count 0 or > BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES, a
 * nodes entry 0, the product of nodes > BEAMFORMER_HIP_MAX_WARP_NODES, count x that product > BEAMFORMER_HIP_MAX_WARP_ENTRIES:
 * BufferOverflow (count first, then -- once nodes is known not to be NULL -- the lattice); field, nodes, node_first or node_step
 * NULL, a field value, a rotation or a node_first that is not finite, a field value of magnitude > BEAMFORMER_HIP_MAX_WARP_DISPLACEMENT,
 * a node_step that is not finite or <= 0 on an axis with more than one node (with one node it is not read), an unknown interpolation
 * or edge, a nonzero imaginary rotation on real frames, a frame of more than 2^31 - 1 voxels, and everything
 * beamformer_hip_score_last_frames refuses, several devices included: InvalidAccess; frames that differ in grid or kind:
 * DataSizeMismatch; a run of `count` frames that does not fit the ring, or that would reuse storage of one of its own source frames:
 * FrameSizeOverflow. */
#define BEAMFORMER_HIP_MAX_WARP_NODES        4096u        /* product of nodes */
#define BEAMFORMER_HIP_MAX_WARP_ENTRIES      32768u       /* count x product of nodes */
#define BEAMFORMER_HIP_MAX_WARP_DISPLACEMENT 65536.0f     /* |component| of a field value, voxels */
typedef enum {
	BeamformerHipWarpInterpolation_Linear = 0,
	BeamformerHipWarpInterpolation_Cubic  = 1,
	BeamformerHipWarpInterpolation_Count
} BeamformerHipWarpInterpolation;
typedef enum {
	BeamformerHipWarpEdge_Zero  = 0,
	BeamformerHipWarpEdge_Clamp = 1,
	BeamformerHipWarpEdge_Count
} BeamformerHipWarpEdge;
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_warp_last_frames(uint32_t count, const float *field, const uint32_t nodes[3],
                                                               const float node_first[3], const float node_step[3],
                                                               const float *rotations, uint32_t interpolation, uint32_t edge,
                                                               uint32_t image_plane_tag, uint32_t *first_frame_id, float *device_ms);

/* The newest frame as ONE of the devices of beamformer_hip_set_devices saw it: its slab's voxels and
 * pairs, its own event times.  (beamformer_hip_get_last_frame_timings reports the ingest device's stage
 * times with the voxel and pair counts of the whole frame and the slowest device's frame time.) */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_get_device_frame_timings(uint32_t device_index, BeamformerHipFrameTimings *out);

/* One device of the set and its share of the newest frame: what a scaling run needs to explain itself.
 * peer_access: 2 = the ingest device (RF arrives from the host / the caller), 1 = direct peer access to the ingest device
 * is enabled (hipDeviceCanAccessPeer said yes and hipDeviceEnablePeerAccess succeeded or was already on: the RF copy crosses
 * one xGMI link), 0 = no peer access (the runtime stages hipMemcpyPeerAsync through host memory: slower, still correct).
 * rf_checksum: sum over the 8-byte words w[i] of the RF this device's newest frame read of w[i] * (i + 1) mod 2^64, computed
 * on the device -- equal on every device of a healthy set. */
typedef struct {
	int32_t  ordinal;             /* HIP device ordinal */
	int32_t  peer_access;
	uint32_t slab_first, slab_count;   /* z planes of the newest frame beamformed here */
	float    peer_copy_ms;        /* the RF copy into this device (0 on the ingest device) */
	float    das_ms, frame_ms;    /* its DAS stage and its whole stage list (HIP events on its compute stream) */
	uint64_t rf_checksum;
	uint64_t rf_bytes;
} BeamformerHipDeviceInfo;
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_get_device_info(uint32_t device_index, BeamformerHipDeviceInfo *out);

/* Frame graphs (BASELINE.json configs[4] names a "hipGraph-captured frame"; the reference records one command
 * list per frame, beamformer_core.c:1570-1620).  When enabled, the stage launches of a frame are captured into a
 * hipGraph, the parameter block's instantiated graph is updated in place from the capture (the frame-ring slot and
 * the RF slot move every frame, so kernel arguments do) and launched as one unit.  Frames are bit-identical either
 * way.  Off by default: measured, a replayed frame is never faster than the <= 6 direct launches it replaces and
 * 4 us slower on 15-us frames (profiles/r02_graph_probe.json), and a graph frame times as ONE segment (reported
 * under DAS) because events cannot be recorded inside it.  One device only; pair counting falls back to direct
 * launches.  beamformer_hip_frame_graph_counts reports how many frames were replayed from a graph and how many
 * graphs had to be instantiated (one per plan unless the stage topology changes). */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_enable_frame_graphs(uint32_t enable);
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_frame_graph_counts(uint64_t *frames_replayed, uint64_t *graphs_instantiated);

/* When enabled, every frame also runs a geometry-only kernel that counts the triples that
 * pass the apodization test (G in BASELINE.md section 4).  Off by default. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_enable_pair_counting(uint32_t enable);

/* min and max over the newest frame of |v| (complex) or v (real).  Build-defined: the
 * reference's shaders/min_max.glsl is dead code (beamformer_core.c:632-637). */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_frame_min_max(float out_min_max[2]);

/* Average of the `count` newest frames (all of one size and kind), written to host memory:
 * the reference's Sum stage -- shaders/sum.glsl applied once per frame, oldest first, with
 * prescale 1/count onto a cleared image (beamformer_core.c:1417-1448).  The reference's
 * planner skips Sum in every pipeline (beamformer_core.c:632-637) and so does this
 * library; the stage is offered here so frame averaging (output_points[3]) has a device
 * implementation.  out_size >= the 64-byte-rounded frame size. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_sum_last_frames(uint32_t count, void *out, uint64_t out_size);

/* Copy of the buffer the newest frame's DAS stage read -- the RF slot when no stage runs before DAS, else the last pre-DAS
 * stage's output -- to host memory: [channel][transmit][sample], channel_count x acquisition_count x das_samples elements
 * (BeamformerHipPlan), f32 or f32 complex as the plan says (iq_pipeline).  Valid until the next push.  Returns 0 when size
 * differs from that, when there is no such frame, or with several devices (beamformer_hip_set_devices).  After a READI image push
 * the buffer its DAS stage read is the one decoded across the acquisitions: channel_count x (readi_group_count x acquisition_count) x
 * das_samples elements, and `size` is judged against that. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_copy_das_input(void *out, uint64_t size);

/* The same for RF frame `frame` of the newest push: a burst's frame `frame` (0: its oldest), each frame of the layout and size above;
 * a single push and a views push hold one RF frame, frame 0.  beamformer_hip_copy_das_input serves the newest frame: after a burst its
 * last one; after a READI image push frame k is what the decode read for RF frame k.  Valid until the next push.  Returns 0 (InvalidAccess) when frame is not below the push's RF frame count, and where
 * beamformer_hip_copy_das_input does. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_copy_das_input_frame(uint32_t frame, void *out, uint64_t size);

/* Display reduction of the newest frame, the step on the far side of the path: the per-voxel
 * intensity the reference's render shader computes (sample_value, shaders/render_3d.frag.glsl:
 * 50-73; defaults threshold 55 dB, gamma 1, dynamic range 50 dB, ui.c:880-883): |v| clamped to
 * 10^(threshold_db/20), normalised, raised to gamma, and -- when db_cutoff > 0 (log scale) --
 * mapped through a db_cutoff-wide dB window.  Writes one float in [0,1] per voxel (x fastest). */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_display_last_frame(float threshold_db, float gamma, float db_cutoff,
                                                                float *out, uint64_t out_floats);

/* The Hilbert stage.  In the reference BeamformerShaderKind_Hilbert is served by an out-of-tree
 * CUDA routine (cuda_hilbert, beamformer_internal.h:233-261) that the snapshot cannot load:
 * capabilities.hilbert is 0 (beamformer.c:262-263) and a pipeline naming the stage is refused with
 * InvalidComputeStage -- which is also what this library does by default.  Enabling this switch
 * makes the stage available with the library's OWN definition (there is nothing to be identical
 * to: parity unpinned): the analytic signal x + j H{x} along samples by a 63-tap type-III FIR
 * Hilbert transformer (Hamming window), real part = the input delayed by 31 samples, the delay added
 * to the DAS time offset; real input only; as in the reference's planner the stage is dropped when
 * the pipeline also demodulates (beamformer_core.c:567) and makes the pipeline IQ (:589). */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_enable_hilbert(uint32_t enable);

/* Select the DAS implementation: 0 = automatic.  Row-column frames whose receive aperture and transmit
 * steering lie along different array axes (separable delays) run the LDS-staged kernels (das_staged.hip /
 * das_staged_real.hip for linear interpolation of IQ / real samples, das_staged_cubic.hip for cubic interpolation of
 * IQ samples: a tile's delay spread inside its LDS window, at least 6 transmits per channel) or else, for linear
 * interpolation, the gather kernel (das_separable.hip); otherwise the per-voxel factored
 * kernel takes RCA-family and FORCES frames with three or more transmits, the gather kernel the remaining
 * separable ones, the general kernel everything else.  1 = always the general kernel, 2 = as automatic but
 * never the LDS-staged kernel, 3 = the LDS-staged kernel wherever its window bound holds (also below 6
 * transmits), 4 = the factored kernel wherever it applies (also ahead of the gather kernel).
 * HERCULES-family frames whose grid is aligned with the array (one lateral transducer coordinate a
 * function of the output row alone) and at least 32 voxels wide run the aligned-grid kernel
 * (das_hercules.hip) in every mode but 1; 6 = that kernel also on narrow grids (idle lanes).
 * Adding 0x10 keeps the general kernel at one thread per voxel for frames it would otherwise
 * split over channels (frames under ~4096 waves of voxels: K waves share 64 voxels, each
 * sums C/K channels, partial sums meet in LDS); adding 0x20 keeps Decode on the O(T^2) kernel
 * where it would run as a fast Walsh-Hadamard transform.  For parity testing of every path. */
typedef enum {
	BeamformerHipDasPath_Automatic        = 0,
	BeamformerHipDasPath_General          = 1,    /* das.hip for every frame */
	BeamformerHipDasPath_NoLdsStaging     = 2,    /* automatic, but das_separable.hip where das_staged.hip would run */
	BeamformerHipDasPath_PreferLdsStaged  = 3,    /* das_staged.hip wherever its window bound holds */
	BeamformerHipDasPath_PreferFactored   = 4,    /* das_factored.hip wherever the index factorises */
	BeamformerHipDasPath_HerculesAnyWidth = 6,    /* das_hercules.hip also on grids narrower than 32 voxels */
	BeamformerHipDasPath_NoChannelSplit   = 0x10, /* flag: general kernel at one thread per voxel for small frames too */
	BeamformerHipDasPath_DenseDecode      = 0x20, /* flag: Decode on the O(T^2) kernel, not the Walsh-Hadamard form */
	BeamformerHipDasPath_TileStaging      = 0x100,/* flag: das_tile.hip (factored kernel, block-wide LDS staging of cubic polynomials) wherever it is supported --
	                                                 automatic on fine grids only */
	BeamformerHipDasPath_NoTileStaging    = 0x200,/* flag: never */
	BeamformerHipDasPath_NoBurstKernel    = 0x400,/* flag: a burst (above) runs the single-frame DAS kernel once per frame also where das_burst.hip would take it */
	BeamformerHipDasPath_NoViewsKernel    = 0x800,/* flag: a views push runs every view's single-frame DAS kernel also where das_views.hip would take it */
	BeamformerHipDasPath_PreferViewsKernel = 0x1000,/* flag: das_views.hip takes the eligible views however few their tiles (for tests) */
	BeamformerHipDasPath_FailViewsDas     = 0x2000,/* flag: a views push (a burst views push, a variants push) FAILS (InvalidAccess) at its DAS stage, after its
	                                                  ids are taken and its frames placed and before anything is launched there -- what a failed launch leaves
	                                                  behind (a tombstone under every id of the push), reachable without a device fault (for tests; no other
	                                                  push is affected) */
	BeamformerHipDasPath_NoVariantsKernel = 0x4000,/* flag: a variants push runs every variant's single-frame DAS kernel also where das_variants.hip would take it */
	BeamformerHipDasPath_PreferVariantsKernel = 0x8000,/* flag: das_variants.hip takes the eligible variants however few their tiles (for tests) */
	BeamformerHipDasPath_WarpDirect       = 0x10000,/* flag: every tile of beamformer_hip_warp_last_frames takes the direct path, also where its source box fits
	                                                   the LDS budget (for tests and measurements: the bytes are the same).  A knob of that one call that merely
	                                                   lives in this mode word: setting or clearing it changes no DAS kernel, but, like every change of the
	                                                   mode, it makes the next push decide its cached DAS routes afresh */
} BeamformerHipDasPath;
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_set_das_path(uint32_t mode);
/* Environment variables the library reads (none is needed in production):
 *   BEAMFORMER_HIP_DEVICE            HIP ordinal of the one-device mode (else LOCAL_RANK, else 0)
 *   BEAMFORMER_HIP_FRAME_RING_BYTES  size of the beamformed-frame ring (default 4 GiB)
 * Diagnostic switches (beamformer_hip_set_hook only -- no environment variable; they select among code paths that ship anyway):
 *   STAGED_SHAPE=u,v,w      the LDS-staged kernels only with 2^u x 2^v voxel tiles and 2^w-sample windows
 *   STAGED_CHECKED          the LDS-staged kernels' range-checked loop for every wave; it also counts window violations
 *                           (BeamformerHipFrameTimings::staged_window_violations)
 *   STAGED_NOUNIFORM        transmit tables in LDS also where the wave-uniform (global table) form applies
 *   STAGED_TABLE_CAP=bytes  largest global transmit table taken (default 2 GiB; 0: always the LDS-table fallback)
 *   DEBUG                   one line per staged plan on stderr
 *   SCRATCH_POISON          both intermediate buffers and the frame's ring slot filled with 0xFF bytes (NaN in binary16 and f32)
 *                           at the start of every frame: an element a stage reads without the frame having written it turns into NaN
 * and two of the frame operations:
 *   GRAM_BOXES_BUDGET=bytes the partials a batch of boxes of beamformer_hip_gram_boxes_last_frames may hold (default 64 MiB): a small
 *                           value makes a handful of small boxes cross a batch boundary (the bytes are the same)
 *   BLEND_SHAPE=0|1         the kernel of beamformer_hip_mix_field_last_frames: 0 the corner nodes outermost, 1 each source loaded once
 *                           for all corners (only where the lattice has one node along y; elsewhere 0 runs); unset: the measured
 *                           default (the bytes are the same) */

/* ---- ZBP acquisition files (external/zemp_bp.h; loader tests/throughput.c:135-374) ----
 * Host only, no device needed.  The reference keeps this loader in its throughput harness;
 * it lives in the library here so every binding gets it. */
typedef struct {
	uint32_t major;                   /* header version: 1 or 2 */
	uint32_t data_kind;               /* BeamformerDataKind of the RF payload */
	uint32_t compression_kind;        /* 0 = none, 1 = zstd (ZBP_DataCompressionKind) */
	uint32_t reserved;
	uint64_t offset, size;            /* payload inside the file; size 0: the payload is the side file <name>_NN.zst */
} BeamformerHipZbpPayload;

/* Fill `out` from the bytes of a .bp file exactly as beamformer_simple_parameters_from_zbp_file
 * (tests/throughput.c:150-374) does: geometry, channel map, per-transmit focal data, emission;
 * the caller still chooses the output grid, f-number, interpolation and compute stages.
 * Every offset in the file is bounds checked.  Returns 0 on failure (see ..._zbp_last_error). */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_zbp_parameters(const void *file_bytes, uint64_t file_size,
                                                            BeamformerSimpleParameters *out,
                                                            BeamformerHipZbpPayload *payload);
/* Read <path> (.bp), fill `out`, and return frame `frame_number`'s RF, decompressed, in a
 * malloc'ed buffer (*rf, *rf_size) to be released with beamformer_hip_zbp_free.  zstd payloads
 * need libzstd.so.1 at run time. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_zbp_load(const char *path, uint32_t frame_number,
                                                      BeamformerSimpleParameters *out, void **rf, uint64_t *rf_size);
BEAMFORMER_LIB_EXPORT void        beamformer_hip_zbp_free(void *rf);
BEAMFORMER_LIB_EXPORT const char *beamformer_hip_zbp_last_error(void);

/* The voxel-grid transform the reference's callers build with das_transform (math.c:831-920):
 * 1-D line, 2-D x-z plane, or 3-D box depending on how many of points[0..2] exceed 1; points
 * are clamped to >= 1 in place.  out16 is column major. */
BEAMFORMER_LIB_EXPORT void beamformer_hip_host_das_transform(const float min_coordinate[3], const float max_coordinate[3],
                                                            int32_t points[3], float out16[16]);

/* ---- host-side introspection (no device needed; used by tests/ to pin the host math
 * against the compiled reference and to check the planner) ---- */

/* Hadamard matrix this library uploads for Decode: order*order floats, row major,
 * Ht[order*j + i] (math.c:35-134).  Returns 0 when no construction exists. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_host_hadamard(uint32_t order, float *out);

/* Filter taps this library generates for a beamformer_create_filter() request
 * (beamformer_core.c:366-398).  Returns the tap count (pairs when *complex_taps), or -1. */
BEAMFORMER_LIB_EXPORT int32_t beamformer_hip_host_filter(const BeamformerFilterParameters *filter, float *taps,
                                                         uint32_t capacity_floats, float *time_delay,
                                                         uint32_t *complex_taps);

typedef struct {
	int32_t kind;                     /* BeamformerShaderKind */
	int32_t in_kind, out_kind;        /* BeamformerDataKind */
	int64_t in_stride[3], out_stride[3];   /* sample, channel, transmit (elements) */
} BeamformerHipPlanStage;
typedef struct {
	uint32_t stage_count;
	BeamformerHipPlanStage stages[BeamformerMaxComputeShaderStages];
	uint32_t das_samples, iq_pipeline;
	float    das_sampling_frequency, das_time_offset;
	float    das_voxel_transform[16];
	uint64_t intermediate_bytes;      /* what the executor allocates (+ 64) for each of its two inter-stage buffers, and a burst's
	                                   * frame stride there: the largest write extent of the plan's stages (csrc/planner.cpp) */
} BeamformerHipPlan;
/* The stage list the library would run for a parameter block (plan_compute_pipeline,
 * beamformer_core.c:553-1013, with the whole channel count as the chunk). */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_describe_plan(uint32_t parameter_slot, BeamformerHipPlan *out);

/* Which DAS kernel the frames of a parameter block run under the current das path mode, and why each kernel ahead of it in the
 * selection order was not taken: the library's ONE table of rules (csrc/das_select.cpp), asked instead of restated.  Needs no
 * device.  path: BeamformerHipFrameTimings::das_path numbering; -1: the pipeline has no DAS stage; -2: an acquisition kind or
 * interpolation mode the shader leaves at zero (the frame is cleared, no kernel). */
typedef struct {
	int32_t  path;
	char     kernel[48];            /* "das_rca_staged_kernel", ... */
	char     name[64];              /* "separable-delay LDS-staged kernel", ... */
	char     declined[8][160];      /* by path number: why that kernel does not run ("" for the one that does) */
	uint32_t tile_shift[3], blocks[3], split_shift;      /* per-voxel kernels (general, factored): block shape and count */
	uint32_t tile_walk;             /* 0 x,y,z; 1 z fastest; 2 y fastest; 3 view plane in XCD-balanced bands; staged kernels: + their flag bits */
	uint32_t row_end_planes;        /* planes of the shard the row-end rule hands to the kernel behind the staged one (BeamformerHipFrameTimings::das_row_end_planes) */
	uint32_t tile_window_samples;   /* block-staged factored kernel (path 5): staged window length */
	uint32_t u_axis, u_shift, v_shift, window_samples, uniform_tables, lds_bytes, threads, channel_chunk;   /* separable-delay kernels: the tile is 2^u_shift voxels
	                                   along the receive axis (voxel axis u_axis) by 2^v_shift along the transmit axis, one plane thick */
	uint32_t hercules_prepared_copy;/* HERCULES kernel: reads the {sample, difference} / polynomial copy of the DAS input */
	float    tile_spread_estimate;  /* factored-kernel frames: the host's upper bound of a 1024-voxel tile's delay spread in samples (what decides
	                                   for or against path 5; the kernel measures the real spread per block and chunk); 0 where not computed */
	uint32_t tile_estimate_shift[3];/* ... and the tile it was computed for */
	uint32_t row_ends;              /* 1: some in-aperture term of the launch may come within reach of an end of its RF row (a host bound, per plane, in
	                                   double precision): the kernel's instantiation WITH the exact row-end evaluation runs (csrc/das_exact.h); 0: the one without */
	int32_t  row_end_path;          /* the kernel (path numbering as above) of the planes the row-end rule re-routed -- of the most of them where
	                                   there is more than one such run --; -1 when row_end_planes is 0 */
} BeamformerHipDasDescription;
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_describe_das(uint32_t parameter_slot, BeamformerHipDasDescription *out);

/* How the RF of a push reaches the RF ring: the library's ONE rule (csrc/executor.cpp: decide_upload), which the push functions follow
 * and this call reports.  Needs no device.  data_size: the bytes of ONE raw frame, as the push calls take it; frame_count: 1 describes
 * beamformer_push_data_with_compute / beamformer_hip_push_device_data_with_compute, 2 and more a burst of that many frames (every
 * push of several frames, and the views and variants pushes of one, follow the burst's rule: the ingest kernel always runs, and the
 * whole upload is measured against the copy-engine threshold); device_pointer: the device address a device-resident push would be
 * given -- the copy width depends on its alignment -- or NULL for host data.
 *   route          BeamformerHipUploadRoute:
 *                  PinnedInPlace     host data under 8 MiB: copied into a pinned slot, which the ingest kernel reads in place;
 *                  CopyEngineDirect  host data of 8 MiB and more already in the mapped layout (identity channel mapping, no row padding,
 *                                    no contrast mode): one H2D copy on the copy stream into the RF ring, no kernel;
 *                  CopyEngineStaged  other host data of 8 MiB and more: H2D into raw staging on the copy stream, then the ingest kernel;
 *                  DeviceBorrowed    device data already in the mapped layout whose plan does not start with DAS: the first stage
 *                                    reads the caller's buffer in place;
 *                  DeviceCopy        ... whose plan starts with DAS: one device-to-device copy into the RF ring;
 *                  DeviceIngest      other device data: the ingest kernel reads the caller's buffer;
 *   ingest_kernel  0 none, 1 ingest_copy_kernel, 2 ingest_a1s2_kernel;
 *   copy_bytes     ingest_copy_kernel: bytes per lane and step, 16, 4 or 2 -- the widest that divides the raw and the mapped row, the
 *                  frame strides of a burst and device_pointer; otherwise 0;
 *   a1s2_base      the scalar type of the data kind, which ingest_a1s2_kernel is instantiated for: 0 int16, 1 float32, 2 float16;
 *   rf_bytes       one frame in the RF ring (what beamformer_hip_get_device_info checksums);
 *   upload_bytes   data_size x frame_count, what the threshold is applied to. */
typedef enum {
	BeamformerHipUploadRoute_PinnedInPlace    = 0,
	BeamformerHipUploadRoute_CopyEngineDirect = 1,
	BeamformerHipUploadRoute_CopyEngineStaged = 2,
	BeamformerHipUploadRoute_DeviceBorrowed   = 3,
	BeamformerHipUploadRoute_DeviceCopy       = 4,
	BeamformerHipUploadRoute_DeviceIngest     = 5,
	BeamformerHipUploadRoute_Count
} BeamformerHipUploadRoute;
typedef struct {
	uint32_t route, ingest_kernel, copy_bytes, a1s2_base;
	uint64_t rf_bytes, upload_bytes;
	char     name[32];              /* "pinned-in-place", "copy-engine-direct", "copy-engine-staged", "device-borrowed", "device-copy", "device-ingest" */
} BeamformerHipUploadDescription;
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_describe_upload(uint32_t parameter_slot, uint32_t data_size, uint32_t frame_count,
                                                             const void *device_pointer, BeamformerHipUploadDescription *out);

/* Diagnostic switches (none is needed in production; listed above, csrc/das_select.h says what each does): set and cleared
 * (value NULL or "") through this call only -- the library reads no environment variable for them.  Returns 0 for an unknown name. */
BEAMFORMER_LIB_EXPORT uint32_t beamformer_hip_set_hook(const char *name, const char *value);

/* Free every device resource; the next call re-initialises. */
BEAMFORMER_LIB_EXPORT void beamformer_hip_shutdown(void);

#ifdef __cplusplus
}
#endif
#endif /* OGL_BEAMFORMER_HIP_H */
