/* lib_api.cpp -- the exported C ABI (include/ogl_beamformer_lib.h, include/ogl_beamformer_hip.h).
 *
 * Every function mirrors the function of the same name in the reference's client library
 * lib/ogl_beamformer_lib.c: same validation, in the same order, with the same error codes.
 * Where the reference writes into a shared-memory parameter block and marks a region dirty
 * (parameter_block_region_upload, lib .c:349-362) this writes into the process-local
 * bf::ParameterBlock and sets the same dirty bit; where it queues work for the server and
 * takes futex locks, this launches on the HIP stream.
 *
 * Parameter functions are pure host state and work without a device; functions that move
 * data or compute need a HIP device and fail with BeamformerLibErrorKind_SharedMemory
 * (the reference's "server unreachable") when there is none.
 */
#include "context.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace bf;

namespace {

/* generated/beamformer.c:538-541 */
const uint8_t contrast_mode_samples[] = {1, 3};

template <typename T> T max_of(T a, T b) { return a > b ? a : b; }

bool check(bool condition, BeamformerLibErrorKind kind)          /* lib_error_check, lib .c:140-148 */
{
	if (!condition) set_error(kind);
	return condition;
}

uint64_t frame_ring_bytes()
{
	Context &c = ctx();
	if (!c.frame_ring_bytes) c.frame_ring_bytes = default_frame_ring_bytes();
	return c.frame_ring_bytes;
}

bool valid_parameter_block(uint32_t block)                       /* lib .c:173-182 */
{
	return check(block < ctx().reserved_parameter_blocks, BeamformerLibErrorKind_ParameterBlockUnallocated);
}

/* lib .c:252-277 */
bool validate_parameters(const BeamformerParameters *bp)
{
	if (!check((int)bp->contrast_mode >= 0 && bp->contrast_mode <= BeamformerContrastMode_Count - 1,
	           BeamformerLibErrorKind_InvalidContrastMode))
		return false;

	uint32_t contrast_raw_sample_count = bp->acquisition_count * bp->sample_count * contrast_mode_samples[bp->contrast_mode];
	if (!check(contrast_raw_sample_count <= bp->raw_data_dimensions[0], BeamformerLibErrorKind_DataSizeMismatch))
		return false;

	uint64_t buffer_size = frame_ring_bytes();
	/* three 31-bit extents times 8 can wrap 64 bits (the reference's u64 product does): a wrapped size would
	 * pass the check below and launch over a grid the frame ring cannot hold, so saturate instead */
	const uint64_t px = (uint64_t)max_of(1, bp->output_points[0]), py = (uint64_t)max_of(1, bp->output_points[1]),
	               pz = (uint64_t)max_of(1, bp->output_points[2]);
	uint64_t frame_size = UINT64_MAX;
	if (px * py <= (UINT64_MAX >> 3) / pz) frame_size = px * py * pz * 8u /* Float32Complex */;
	uint64_t incoherent_size = frame_size / 2;
	if (bp->coherency_weighting) buffer_size -= incoherent_size;
	return check(frame_size <= buffer_size, BeamformerLibErrorKind_FrameSizeOverflow);
}

/* lib .c:279-311; capabilities.hilbert is 0 here as in the reference (beamformer.c:262-263) */
bool validate_pipeline(const int32_t *shaders, uint32_t shader_count, BeamformerDataKind data_kind)
{
	if (!check((int)data_kind >= 0 && data_kind <= BeamformerDataKind_Count - 1, BeamformerLibErrorKind_InvalidDataKind))
		return false;
	if (!check(shader_count <= BeamformerMaxComputeShaderStages, BeamformerLibErrorKind_ComputeStageOverflow))
		return false;
	for (uint32_t i = 0; i < shader_count; i++) {
		bool stage_ok = shaders[i] >= BeamformerShaderKind_ComputeFirst && shaders[i] <= BeamformerShaderKind_ComputeLast;
		if (!check(stage_ok, BeamformerLibErrorKind_InvalidComputeStage)) return false;
		if (shaders[i] == BeamformerShaderKind_Hilbert &&
		    !check(ctx().hilbert_enabled, BeamformerLibErrorKind_InvalidComputeStage))     /* capabilities.hilbert */
			return false;
		if (shaders[i] == BeamformerShaderKind_Demodulate &&
		    !check(!bf_kind_complex[data_kind], BeamformerLibErrorKind_InvalidDemodulationDataKind))
			return false;
	}
	/* the reference tests shaders[0] whatever shader_count is (lib .c:305-309): an empty pipeline
	 * passes when the caller's array happens to start with Decode or Demodulate.  Kept as is --
	 * callers pass the 16-entry array of BeamformerSimpleParameters -- and an empty plan is
	 * legal here (no stage runs, the frame stays zero). */
	bool start_ok = shaders && (shaders[0] == BeamformerShaderKind_Demodulate ||
	                            shaders[0] == BeamformerShaderKind_Decode);
	return check(start_ok, BeamformerLibErrorKind_InvalidStartShader);
}

/* One RF frame of `size` bytes at `data` against a parameter block (beamformer_push_data_base, lib .c:503-511).  The reference does this
 * arithmetic in u32; a product that wraps there passes its check and then reads far outside the caller's buffer.  Same checks and
 * error codes, in u64: sizes the reference accepts without wrapping are judged identically, wrapped ones are refused. */
bool valid_rf_frame(const ParameterBlock &pb, const void *data, uint32_t size)
{
	const BeamformerParameters &bp = pb.parameters;
	const uint64_t max_rf_size = frame_ring_bytes() / 3;             /* capabilities.max_rf_data_size */
	const uint64_t bytes    = (uint64_t)bf_kind_byte_size[pb.data_kind];
	const uint64_t rf_size  = (uint64_t)bp.acquisition_count * bp.sample_count * bp.channel_count * bytes;
	const uint64_t raw_size = (uint64_t)bp.raw_data_dimensions[0] * bp.raw_data_dimensions[1] * bytes;
	if (!check(data != nullptr, BeamformerLibErrorKind_BufferOverflow)) return false;
	if (!check(rf_size <= max_rf_size && rf_size <= UINT32_MAX, BeamformerLibErrorKind_RFDataSizeOverflow)) return false;
	if (!check(rf_size <= size && (uint64_t)size == raw_size, BeamformerLibErrorKind_DataSizeMismatch)) return false;
	if (!check(rf_size > 0, BeamformerLibErrorKind_DataSizeMismatch)) return false;
	/* the ingest walks channel_mapping[0 .. channel_count): bound it before anything indexes with it */
	return check(bp.channel_count <= BeamformerMaxChannelCount && bp.acquisition_count <= BeamformerMaxEmissionsCount,
	             BeamformerLibErrorKind_DataSizeMismatch);
}

/* a multi-frame push (`what`) is not sharded over the devices of beamformer_hip_set_devices */
bool on_one_device(const char *what)
{
	Context &c = ctx();
	if (c.requested_count <= 1 && !(c.device_ready && c.device_count > 1)) return true;
	std::fprintf(stderr, "[beamformer] a %s runs on one device: refused with the %u devices of beamformer_hip_set_devices\n", what,
	             c.device_ready ? c.device_count : c.requested_count);
	return set_error(BeamformerLibErrorKind_InvalidAccess);
}

/* the block's resolved plan, or InvalidComputeStage */
bool resolved_plan(const ParameterBlock &pb, Plan &plan)
{
	std::string error;
	return check(build_plan(pb, plan, error, ctx().hilbert_enabled), BeamformerLibErrorKind_InvalidComputeStage);
}

/* a multi-frame push's whole run of frames in the frame ring (context.h: frame_run_bytes; needs the block's plan, no device) */
bool run_fits_the_ring(const ParameterBlock &pb, const BeamformerHipView *views, uint32_t count, uint32_t per_view = 1)
{
	Plan plan;
	if (!resolved_plan(pb, plan)) return false;
	const uint32_t points[3] = {plan.output_points[0], plan.output_points[1], pb.shard_z_count ? pb.shard_z_count : plan.output_points[2]};
	uint64_t total;
	return check(frame_run_bytes(points, views, count, plan.iq_pipeline ? 8u : 4u, frame_ring_bytes(), total, per_view), BeamformerLibErrorKind_FrameSizeOverflow);
}

/* the RF frames of a burst, a sweep, an image, a burst views push: a count the ABI's tables hold */
static_assert(BEAMFORMER_HIP_MAX_BURST_FRAMES <= BeamformerMaxBacklogFrames, "every frame of a burst keeps its frame record");
bool valid_burst_count(uint32_t frame_count)
{
	return check(frame_count != 0 && frame_count <= BEAMFORMER_HIP_MAX_BURST_FRAMES, BeamformerLibErrorKind_BufferOverflow);
}

/* The last checks of every multi-frame push (`what`), after those of its own arguments: one device; `whole_grid` (a push of views or
 * variants; `item`: one of them) no output shard on the block; the RF frame; `count` frames in the ring, of the block's grid or --
 * `views` given -- frame k of views[k / per_view]'s; a device.  Everything that needs no device is judged before the device is touched,
 * so that a malformed push is refused the same way on a machine without one. */
bool multi_push_ready(const char *what, const char *item, uint32_t slot, const void *data, uint32_t frame_size, const BeamformerHipView *views, uint32_t count,
                      uint32_t per_view = 1)
{
	const ParameterBlock &pb = ctx().blocks[slot];
	if (!on_one_device(what)) return false;
	if (item && pb.shard_z_count) {
		std::fprintf(stderr, "[beamformer] a %s is not sharded: refused with the output shard set on parameter block %u\n", item, slot);
		return set_error(BeamformerLibErrorKind_InvalidAccess);
	}
	return valid_rf_frame(pb, data, frame_size) && run_fits_the_ring(pb, views, count, per_view) && ensure_device();
}

bool push_data_common(const void *data, uint32_t data_size, uint32_t image_plane_tag, uint32_t slot, bool on_device)
{
	Context &c = ctx();
	if (!ensure_device()) return false;
	if (!check(image_plane_tag < BeamformerViewPlaneTag_Count, BeamformerLibErrorKind_InvalidImagePlane)) return false;
	if (!check(slot < c.reserved_parameter_blocks, BeamformerLibErrorKind_ParameterBlockUnallocated)) return false;
	if (!valid_rf_frame(c.blocks[slot], data, data_size)) return false;
	return push_rf_and_compute(slot, data, data_size, on_device);
}

/* A burst: the single push's checks per frame (one geometry: once), then what must hold for the burst as a whole. */
bool push_burst_common(const void *data, uint32_t frame_size, uint32_t frame_count, uint32_t image_plane_tag, uint32_t slot, bool on_device)
{
	Context &c = ctx();
	if (frame_count == 1) return push_data_common(data, frame_size, image_plane_tag, slot, on_device);
	if (!valid_burst_count(frame_count)) return false;
	if (!check(image_plane_tag < BeamformerViewPlaneTag_Count, BeamformerLibErrorKind_InvalidImagePlane)) return false;
	if (!check(slot < c.reserved_parameter_blocks, BeamformerLibErrorKind_ParameterBlockUnallocated)) return false;
	if (!multi_push_ready("burst", nullptr, slot, data, frame_size, nullptr, frame_count)) return false;
	return push_burst(slot, data, frame_size, frame_count, nullptr, on_device);
}

/* A READI sweep's block and group list, no device needed: the block beamforms READI (FORCES / UFORCES with readi_group_count > 1), else
 * InvalidAccess with a line on stderr; every group id is below readi_group_count, else InvalidComputeStage -- what a single push of a
 * block with that readi_group gets (the planner refuses the block: planner.cpp).  `out`: the frame_count ids, groups == null:
 * (block.readi_group + k) % readi_group_count. */
bool resolve_readi_groups(uint32_t slot, const uint32_t *groups, uint32_t frame_count, std::vector<uint32_t> &out)
{
	Context &c = ctx();
	if (!valid_burst_count(frame_count)) return false;
	if (!check(slot < c.reserved_parameter_blocks, BeamformerLibErrorKind_ParameterBlockUnallocated)) return false;
	const BeamformerParameters &bp = c.blocks[slot].parameters;
	const bool forces = bp.acquisition_kind == BeamformerAcquisitionKind_FORCES || bp.acquisition_kind == BeamformerAcquisitionKind_UFORCES;
	if (!forces || bp.readi_group_count <= 1) {
		std::fprintf(stderr, "[beamformer] a READI sweep needs a FORCES / UFORCES block with readi_group_count > 1: refused (acquisition kind %d, readi_group_count %u)\n",
		             (int)bp.acquisition_kind, bp.readi_group_count);
		return set_error(BeamformerLibErrorKind_InvalidAccess);
	}
	const uint32_t G = bp.readi_group_count;
	out.resize(frame_count);
	for (uint32_t k = 0; k < frame_count; k++) {
		out[k] = groups ? groups[k] : (uint32_t)(((uint64_t)bp.readi_group + k) % G);
		if (!check(out[k] < G, BeamformerLibErrorKind_InvalidComputeStage)) return false;
	}
	return true;
}

/* A READI sweep: the burst's checks and the list's, all before the device is touched; frame_count == 1 goes the same way. */
bool push_readi_sweep_common(const void *data, uint32_t frame_size, uint32_t frame_count, const uint32_t *groups, uint32_t image_plane_tag, uint32_t slot,
                             bool on_device)
{
	if (!valid_burst_count(frame_count)) return false;
	if (!check(image_plane_tag < BeamformerViewPlaneTag_Count, BeamformerLibErrorKind_InvalidImagePlane)) return false;
	std::vector<uint32_t> ids;
	if (!resolve_readi_groups(slot, groups, frame_count, ids)) return false;
	if (!multi_push_ready("READI sweep", nullptr, slot, data, frame_size, nullptr, frame_count)) return false;
	return push_burst(slot, data, frame_size, frame_count, ids.data(), on_device);
}

/* A READI image push's block, list and count, no device needed: the sweep's checks (resolve_readi_groups), then what the derived block
 * -- FORCES with readi_group_count x acquisition_count transmits -- must satisfy: the emission limit (InvalidAccess, with a line on
 * stderr) and a decoded DAS input under 4 GiB (RFDataSizeOverflow).  `derived` / `derived_plan`: that block and its plan. */
bool resolve_readi_image(uint32_t slot, const uint32_t *groups, uint32_t frame_count, std::vector<uint32_t> &ids, ParameterBlock &derived, Plan &derived_plan)
{
	Context &c = ctx();
	if (!resolve_readi_groups(slot, groups, frame_count, ids)) return false;
	const ParameterBlock &pb = c.blocks[slot];
	const BeamformerParameters &bp = pb.parameters;
	const uint64_t transmits = (uint64_t)bp.readi_group_count * bp.acquisition_count;
	if (transmits > BeamformerMaxEmissionsCount) {
		std::fprintf(stderr, "[beamformer] a READI image needs readi_group_count x acquisition_count <= %d transmits: refused (%u x %u)\n",
		             (int)BeamformerMaxEmissionsCount, bp.readi_group_count, bp.acquisition_count);
		return set_error(BeamformerLibErrorKind_InvalidAccess);
	}
	Plan plan;
	if (!resolved_plan(pb, plan)) return false;
	derive_readi_image(pb, plan, derived, derived_plan);
	const uint64_t decoded = (uint64_t)plan.channels * transmits * plan.das_samples * (plan.iq_pipeline ? 8u : 4u);
	return check(decoded < (1ull << 32), BeamformerLibErrorKind_RFDataSizeOverflow);
}

/* A READI image push: the sweep's checks and the derived block's, all before the device is touched; ONE frame must fit the ring. */
bool push_readi_image_common(const void *data, uint32_t frame_size, uint32_t frame_count, const uint32_t *groups, uint32_t image_plane_tag, uint32_t slot,
                             bool on_device)
{
	if (!valid_burst_count(frame_count)) return false;
	if (!check(image_plane_tag < BeamformerViewPlaneTag_Count, BeamformerLibErrorKind_InvalidImagePlane)) return false;
	std::vector<uint32_t> ids;
	ParameterBlock derived;
	Plan derived_plan;
	if (!resolve_readi_image(slot, groups, frame_count, ids, derived, derived_plan)) return false;
	if (!multi_push_ready("READI image push", nullptr, slot, data, frame_size, nullptr, 1)) return false;
	return push_readi_image(slot, data, frame_size, frame_count, ids.data(), on_device);
}

/* What a views call must satisfy that needs neither the RF nor a device: the count, the list, the block, every view's tag and extents. */
bool validate_views(const BeamformerHipView *views, uint32_t view_count, uint32_t slot)
{
	Context &c = ctx();
	if (!check(view_count != 0 && view_count <= BEAMFORMER_HIP_MAX_VIEWS, BeamformerLibErrorKind_BufferOverflow)) return false;
	if (!check(views != nullptr, BeamformerLibErrorKind_InvalidAccess)) return false;
	if (!check(slot < c.reserved_parameter_blocks, BeamformerLibErrorKind_ParameterBlockUnallocated)) return false;
	for (uint32_t k = 0; k < view_count; k++) {
		if (!check(views[k].image_plane_tag < BeamformerViewPlaneTag_Count, BeamformerLibErrorKind_InvalidImagePlane)) return false;
		const uint32_t *n = views[k].output_points;
		if (!check(n[0] != 0 && n[1] != 0 && n[2] != 0, BeamformerLibErrorKind_InvalidAccess)) return false;
	}
	return true;
}

static_assert(BEAMFORMER_HIP_MAX_VIEWS <= BeamformerMaxBacklogFrames, "every view of a push keeps its frame record");

/* A views push: what must hold for the views, then the single push's checks of the RF (once). */
bool push_views_common(const void *data, uint32_t data_size, const BeamformerHipView *views, uint32_t view_count, uint32_t slot, bool on_device)
{
	if (!validate_views(views, view_count, slot)) return false;
	if (!multi_push_ready("views push", "view", slot, data, data_size, views, view_count)) return false;
	return push_views(slot, data, data_size, views, view_count, on_device);
}

/* What a burst views call must satisfy that needs neither the RF nor a device: both counts, their product (every frame keeps its record),
 * then the views push's checks of the list. */
bool validate_burst_views(uint32_t frame_count, const BeamformerHipView *views, uint32_t view_count, uint32_t slot)
{
	if (!valid_burst_count(frame_count)) return false;
	if (!check(view_count != 0 && view_count <= BEAMFORMER_HIP_MAX_VIEWS, BeamformerLibErrorKind_BufferOverflow)) return false;
	if (!check((uint64_t)frame_count * view_count <= BeamformerMaxBacklogFrames, BeamformerLibErrorKind_BufferOverflow)) return false;
	return validate_views(views, view_count, slot);
}

/* A burst views push: the burst's checks of the RF, the views push's of the views, then the whole run against the ring -- all before the
 * device is touched; frame_count == 1 goes the same way. */
bool push_burst_views_common(const void *data, uint32_t frame_size, uint32_t frame_count, const BeamformerHipView *views, uint32_t view_count, uint32_t slot,
                             bool on_device)
{
	if (!validate_burst_views(frame_count, views, view_count, slot)) return false;
	if (!multi_push_ready("burst views push", "view", slot, data, frame_size, views, frame_count * view_count, frame_count)) return false;
	return push_burst_views(slot, data, frame_size, frame_count, views, view_count, on_device);
}

static_assert(BEAMFORMER_HIP_MAX_VARIANTS <= BeamformerMaxBacklogFrames, "every variant of a push keeps its frame record");

/* What a variants call must satisfy that needs neither the RF nor a device: the count, the list, the block, every variant's fields. */
bool validate_variants(const BeamformerHipDasVariant *variants, uint32_t variant_count, uint32_t slot)
{
	Context &c = ctx();
	if (!check(variant_count != 0 && variant_count <= BEAMFORMER_HIP_MAX_VARIANTS, BeamformerLibErrorKind_BufferOverflow)) return false;
	if (!check(variants != nullptr, BeamformerLibErrorKind_InvalidAccess)) return false;
	if (!check(slot < c.reserved_parameter_blocks, BeamformerLibErrorKind_ParameterBlockUnallocated)) return false;
	for (uint32_t k = 0; k < variant_count; k++) {
		const BeamformerHipDasVariant &v = variants[k];
		if (std::isfinite(v.speed_of_sound) && std::isfinite(v.time_offset) && std::isfinite(v.f_number) && v.speed_of_sound > 0.0f) continue;
		std::fprintf(stderr, "[beamformer] variant %u needs finite fields and a speed of sound above 0: refused (speed_of_sound %g, time_offset %g, f_number %g)\n",
		             k, (double)v.speed_of_sound, (double)v.time_offset, (double)v.f_number);
		return set_error(BeamformerLibErrorKind_InvalidAccess);
	}
	return true;
}

std::vector<DasVariant> das_variants(const BeamformerHipDasVariant *variants, uint32_t variant_count)
{
	std::vector<DasVariant> out(variant_count);
	for (uint32_t k = 0; k < variant_count; k++) out[k] = DasVariant{variants[k].speed_of_sound, variants[k].time_offset, variants[k].f_number};
	return out;
}

/* A variants push: the list's checks, the single push's checks of the RF (once), then what must hold for the run of frames. */
bool push_variants_common(const void *data, uint32_t data_size, const BeamformerHipDasVariant *variants, uint32_t variant_count, uint32_t image_plane_tag,
                          uint32_t slot, bool on_device)
{
	if (!check(variant_count != 0 && variant_count <= BEAMFORMER_HIP_MAX_VARIANTS, BeamformerLibErrorKind_BufferOverflow)) return false;
	if (!check(image_plane_tag < BeamformerViewPlaneTag_Count, BeamformerLibErrorKind_InvalidImagePlane)) return false;
	if (!validate_variants(variants, variant_count, slot)) return false;
	if (!multi_push_ready("variants push", "variant", slot, data, data_size, nullptr, variant_count)) return false;
	return push_variants(slot, data, data_size, das_variants(variants, variant_count).data(), variant_count, on_device);
}

template <typename T>
uint32_t push_array(T *dst, size_t dst_count, const T *src, uint32_t count, uint32_t elements, uint32_t block, uint32_t dirty)
{
	/* X-macro upload functions, lib .c:438-456 */
	if (!check(count <= dst_count, BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!valid_parameter_block(block)) return 0;
	std::memcpy(dst, src, sizeof(T) * count * elements);
	ctx().blocks[block].dirty |= dirty;
	return 1;
}

} // namespace

extern "C" {

uint32_t beamformer_get_api_version(void) { return BEAMFORMER_SHARED_MEMORY_VERSION; }

const char *beamformer_error_string(BeamformerLibErrorKind kind)
{
	static const char *table[] = {
		"None",
		"host-library version mismatch",
		"library in invalid state",
		"parameter block count overflow",
		"push to unallocated parameter block",
		"compute stage overflow",
		"invalid compute shader stage",
		"starting shader not Decode or Demodulate",
		"data kind for demodulation not Int16 or Float",
		"invalid image plane",
		"invalid filter kind",
		"invalid data kind",
		"invalid contrast mode",
		"passed buffer size exceeds available space",
		"data size doesn't match the size specified in parameters",
		"work queue full",
		"not enough space for data export",
		"failed to open shared memory region",
		"failed to acquire lock within timeout period",
		"maximum frame size exceeded",
		"raw rf size exceeds available GPU space",
		"invalid error kind",
	};
	const unsigned last = sizeof(table) / sizeof(*table) - 1;
	unsigned index = (unsigned)kind;
	return table[index < last ? index : last];
}

BeamformerLibErrorKind beamformer_get_last_error(void) { return ctx().last_error; }
const char *beamformer_get_last_error_string(void)      { return beamformer_error_string(ctx().last_error); }
void beamformer_set_global_timeout(uint32_t timeout_ms) { ctx().timeout_ms = (int32_t)timeout_ms; }

uint32_t beamformer_reserve_parameter_blocks(uint32_t count)
{
	if (!check(count <= BeamformerMaxParameterBlocks, BeamformerLibErrorKind_ParameterBlockOverflow)) return 0;
	ctx().reserved_parameter_blocks = count;
	return 1;
}

uint64_t beamformer_maximum_rf_data_size(void)
{
	if (!ensure_device()) return UINT64_MAX;
	return frame_ring_bytes() / 3;
}

uint64_t beamformer_maximum_frames_for_parameters(BeamformerParameters *bp)
{
	if (!validate_parameters(bp)) return UINT64_MAX;
	uint64_t buffer_size = frame_ring_bytes();
	uint64_t frame_size  = (uint64_t)max_of(1, bp->output_points[0]) * (uint64_t)max_of(1, bp->output_points[1])
	                       * (uint64_t)max_of(1, bp->output_points[2]) * 8u;
	if (bp->coherency_weighting) buffer_size -= frame_size / 2;
	return buffer_size / frame_size;
}

uint64_t beamformer_maximum_frames_for_simple_parameters(BeamformerSimpleParameters *bp)
{
	return beamformer_maximum_frames_for_parameters((BeamformerParameters *)bp);
}

uint32_t beamformer_set_pipeline_stage_parameters_at(uint32_t stage_index, int32_t parameter, uint32_t block)
{
	if (!valid_parameter_block(block)) return 0;
	ParameterBlock &pb = ctx().blocks[block];
	pb.filter_slots[stage_index % BeamformerMaxComputeShaderStages] = (uint8_t)parameter;   /* lib .c:364-374 */
	pb.dirty |= Dirty_ComputePipeline;
	return 1;
}

uint32_t beamformer_set_pipeline_stage_parameters(uint32_t stage_index, int32_t parameter)
{
	return beamformer_set_pipeline_stage_parameters_at(stage_index, parameter, 0);
}

uint32_t beamformer_push_pipeline_at(int32_t *shaders, uint32_t shader_count, BeamformerDataKind data_kind, uint32_t block)
{
	if (!validate_pipeline(shaders, shader_count, data_kind)) return 0;
	if (!valid_parameter_block(block)) return 0;
	ParameterBlock &pb = ctx().blocks[block];
	std::memcpy(pb.shaders, shaders, sizeof(*shaders) * shader_count);
	pb.shader_count = shader_count;
	pb.data_kind    = data_kind;
	pb.dirty |= Dirty_ComputePipeline;
	return 1;
}

uint32_t beamformer_push_pipeline(int32_t *shaders, uint32_t shader_count, BeamformerDataKind data_kind)
{
	return beamformer_push_pipeline_at(shaders, shader_count, data_kind, 0);
}

uint32_t beamformer_create_filter(BeamformerFilterParameters *filter, uint8_t filter_slot, uint8_t parameter_block)
{
	if (!check((int)filter->kind >= 0 && filter->kind < BeamformerFilterKind_Count, BeamformerLibErrorKind_InvalidFilterKind))
		return 0;
	/* lib .c:421-422: slot and block wrap instead of failing */
	ParameterBlock &pb = ctx().blocks[parameter_block % BeamformerMaxParameterBlocks];
	pb.filters[filter_slot % BeamformerFilterSlots] = *filter;
	pb.dirty |= Dirty_Filters;
	return 1;
}

uint32_t beamformer_push_channel_mapping_at(int16_t *mapping, uint32_t count, uint32_t block)
{
	return push_array(ctx().blocks[block % BeamformerMaxParameterBlocks].channel_mapping, (size_t)BeamformerMaxChannelCount,
	                  mapping, count, 1, block, Dirty_ChannelMapping);
}
uint32_t beamformer_push_channel_mapping(int16_t *mapping, uint32_t count) { return beamformer_push_channel_mapping_at(mapping, count, 0); }

uint32_t beamformer_push_sparse_elements_at(int16_t *elements, uint32_t count, uint32_t block)
{
	return push_array(ctx().blocks[block % BeamformerMaxParameterBlocks].sparse_elements, (size_t)BeamformerMaxChannelCount,
	                  elements, count, 1, block, Dirty_SparseElements);
}
uint32_t beamformer_push_sparse_elements(int16_t *elements, uint32_t count) { return beamformer_push_sparse_elements_at(elements, count, 0); }

uint32_t beamformer_push_focal_vectors_at(float *vectors, uint32_t count, uint32_t block)
{
	return push_array(&ctx().blocks[block % BeamformerMaxParameterBlocks].focal_vectors[0][0], (size_t)BeamformerMaxChannelCount,
	                  vectors, count, 2, block, Dirty_FocalVectors);
}
uint32_t beamformer_push_focal_vectors(float *vectors, uint32_t count) { return beamformer_push_focal_vectors_at(vectors, count, 0); }

uint32_t beamformer_push_transmit_receive_orientations_at(uint8_t *values, uint32_t count, uint32_t block)
{
	return push_array(ctx().blocks[block % BeamformerMaxParameterBlocks].transmit_receive_orientations,
	                  (size_t)BeamformerMaxChannelCount, values, count, 1, block, Dirty_Orientations);
}
uint32_t beamformer_push_transmit_receive_orientations(uint8_t *values, uint32_t count)
{
	return beamformer_push_transmit_receive_orientations_at(values, count, 0);
}

uint32_t beamformer_push_parameters_at(BeamformerParameters *bp, uint32_t block)
{
	if (!validate_parameters(bp)) return 0;
	if (!valid_parameter_block(block)) return 0;
	ParameterBlock &pb = ctx().blocks[block];
	std::memcpy(&pb.parameters, bp, sizeof(*bp));
	pb.dirty |= Dirty_Parameters;
	return 1;
}
uint32_t beamformer_push_parameters(BeamformerParameters *bp) { return beamformer_push_parameters_at(bp, 0); }

/* lib .c:620-646 */
uint32_t beamformer_push_simple_parameters_at(BeamformerSimpleParameters *bp, uint32_t block)
{
	float focal_vectors[BeamformerMaxEmissionsCount][2];
	for (uint32_t i = 0; i < BeamformerMaxEmissionsCount; i++) {
		focal_vectors[i][0] = bp->steering_angles[i];
		focal_vectors[i][1] = bp->focal_depths[i];
	}
	uint32_t result = 1;
	result &= beamformer_push_parameters_at((BeamformerParameters *)bp, block);
	result &= beamformer_push_pipeline_at(bp->compute_stages, bp->compute_stages_count, bp->data_kind, block);
	result &= beamformer_push_channel_mapping_at(bp->channel_mapping, bp->channel_count, block);
	result &= beamformer_push_focal_vectors_at(&focal_vectors[0][0], BeamformerMaxEmissionsCount, block);
	result &= beamformer_push_transmit_receive_orientations_at(bp->transmit_receive_orientations, bp->acquisition_count, block);
	if (bp->acquisition_kind == BeamformerAcquisitionKind_UFORCES || bp->acquisition_kind == BeamformerAcquisitionKind_UHERCULES)
		result &= beamformer_push_sparse_elements_at(bp->sparse_elements, bp->acquisition_count, block);
	for (uint32_t stage = 0; stage < bp->compute_stages_count && stage < BeamformerMaxComputeShaderStages; stage++)
		result &= beamformer_set_pipeline_stage_parameters_at(stage, bp->compute_stage_parameters[stage], block);
	return result;
}
uint32_t beamformer_push_simple_parameters(BeamformerSimpleParameters *bp) { return beamformer_push_simple_parameters_at(bp, 0); }

uint32_t beamformer_push_data_with_compute(void *data, uint32_t data_size, uint32_t image_plane_tag, uint32_t parameter_slot)
{
	return push_data_common(data, data_size, image_plane_tag, parameter_slot, false);
}

uint32_t beamformer_get_last_frames(void *out_data, uint64_t out_data_size, uint32_t count)
{
	if (!(out_data && out_data_size && count)) return 0;         /* lib .c:700: fails without an error code */
	if (!ensure_device()) return 0;
	return export_last_frames(out_data, out_data_size, count, ctx().timeout_ms);
}

/* lib .c:704-736.  The reference ignores its timeout_ms argument and waits with the global
 * timeout; a non-zero argument is honoured here (superset). */
uint32_t beamformer_beamform_data(BeamformerSimpleParameters *bp, void *data, uint32_t data_size,
                                  void *out_data, int32_t timeout_ms)
{
	uint32_t result = beamformer_push_simple_parameters(bp);
	if (!result) return 0;

	bool complex_out = false;
	for (uint32_t stage = 0; stage < bp->compute_stages_count && stage < BeamformerMaxComputeShaderStages; stage++)
		complex_out |= bp->compute_stages[stage] == BeamformerShaderKind_Demodulate ||
		               bp->compute_stages[stage] == BeamformerShaderKind_Hilbert;
	uint64_t output_size = (uint64_t)max_of(1, bp->output_points[0]) * (uint64_t)max_of(1, bp->output_points[1])
	                       * (uint64_t)max_of(1, bp->output_points[2]) * sizeof(float);
	if (complex_out) output_size *= 2;

	result = beamformer_push_data_with_compute(data, data_size, 0, 0);
	if (result && out_data) {
		if (!ensure_device()) return 0;
		int32_t wait = timeout_ms != 0 ? timeout_ms : ctx().timeout_ms;
		result = export_last_frames(out_data, output_size, 1, wait);
	}
	return result;
}

uint32_t beamformer_compute_timings(BeamformerComputeStatsTable *output, int32_t timeout_ms)
{
	if (!ensure_device()) return 0;
	if (!wait_for_frames(timeout_ms)) return 0;
	return fill_stats_table(output);
}

int32_t beamformer_live_parameters_get_dirty_flag(void)
{
	Context &c = ctx();
	for (int flag = 0; flag < 32; flag++)
		if (c.live_dirty_flags & (1u << flag)) { c.live_dirty_flags &= ~(1u << flag); return flag; }
	return -1;
}

BeamformerLiveImagingParameters *beamformer_get_live_parameters(void) { return &ctx().live; }

uint32_t beamformer_set_live_parameters(BeamformerLiveImagingParameters *params)
{
	std::memcpy(&ctx().live, params, sizeof(*params));
	return 1;
}

/* ---------------- MI355X extensions (include/ogl_beamformer_hip.h) ---------------- */

uint32_t beamformer_hip_set_device(int32_t device_index)
{
	Context &c = ctx();
	if (c.device_ready) return check(c.device_count == 1 && c.devices[0].device == device_index, BeamformerLibErrorKind_InvalidAccess);
	c.requested_devices[0] = device_index;
	c.requested_count = 1;
	return 1;
}

int32_t beamformer_hip_get_device(void)
{
	Context &c = ctx();
	return c.device_ready ? c.devices[0].device : (c.requested_count ? c.requested_devices[0] : -1);
}

uint32_t beamformer_hip_set_devices(const int32_t *device_indices, uint32_t count)
{
	Context &c = ctx();
	if (!check(device_indices != nullptr && count >= 1 && count <= kMaxDevices, BeamformerLibErrorKind_InvalidAccess)) return 0;
	if (c.device_ready) {
		/* like beamformer_hip_set_device: afterwards only the set already in use is accepted */
		bool same = c.device_count == count;
		for (uint32_t i = 0; same && i < count; i++) same = c.devices[i].device == device_indices[i];
		return check(same, BeamformerLibErrorKind_InvalidAccess);
	}
	for (uint32_t i = 0; i < count; i++) {
		if (!check(device_indices[i] >= 0, BeamformerLibErrorKind_InvalidAccess)) return 0;
		c.requested_devices[i] = device_indices[i];
	}
	c.requested_count = count;
	return 1;
}

uint32_t beamformer_hip_get_device_count(void)
{
	Context &c = ctx();
	return c.device_ready ? c.device_count : (c.requested_count ? c.requested_count : 1u);
}

uint32_t beamformer_hip_get_device_frame_timings(uint32_t device_index, BeamformerHipFrameTimings *out)
{
	if (!ensure_device()) return 0;
	return device_frame_timings(device_index, out);
}

uint32_t beamformer_hip_get_device_info(uint32_t device_index, BeamformerHipDeviceInfo *out)
{
	if (!check(out != nullptr, BeamformerLibErrorKind_InvalidAccess) || !ensure_device()) return 0;
	return device_info(device_index, out);
}

uint32_t beamformer_hip_set_stream(void *hip_stream)
{
	Context &c = ctx();
	/* a stream belongs to one device: with several devices the library keeps to its own streams */
	if (!check(beamformer_hip_get_device_count() == 1 || hip_stream == nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	Device &d = c.devices[0];
	if (hip_stream) {
		/* a stream of another device would have every kernel of the library enqueued against buffers it cannot reach: refuse it.
		 * The device the library runs on: the one in use, else the one asked for, else what ensure_device will pick. */
		int wanted = c.device_ready ? d.device : (c.requested_count ? c.requested_devices[0] : -1);
		if (wanted < 0) {
			const char *e = std::getenv("BEAMFORMER_HIP_DEVICE");
			if (!e) e = std::getenv("LOCAL_RANK");
			wanted = e ? std::atoi(e) : 0;
		}
		int owner = -1;
		if (!check(hipStreamGetDevice((hipStream_t)hip_stream, &owner) == hipSuccess && owner == wanted, BeamformerLibErrorKind_InvalidAccess)) {
			(void)hipGetLastError();
			return 0;
		}
	}
	if (c.device_ready && d.stream) (void)hipStreamSynchronize(d.stream);   /* keep frames ordered across the switch */
	d.stream = hip_stream ? (hipStream_t)hip_stream : d.own_stream;
	return 1;
}

uint32_t beamformer_hip_set_output_shard(uint32_t parameter_slot, uint32_t z_first, uint32_t z_count)
{
	if (!valid_parameter_block(parameter_slot)) return 0;
	ParameterBlock &pb = ctx().blocks[parameter_slot];
	uint32_t z_total = (uint32_t)max_of(1, pb.parameters.output_points[2]);
	if (z_count && !check(z_first < z_total && z_count <= z_total - z_first, BeamformerLibErrorKind_FrameSizeOverflow)) return 0;
	pb.shard_z_first = z_count ? z_first : 0;
	pb.shard_z_count = z_count;
	pb.dirty |= Dirty_Shard;
	return 1;
}

uint32_t beamformer_hip_push_device_data_with_compute(const void *device_data, uint32_t size,
                                                      uint32_t image_plane_tag, uint32_t parameter_slot)
{
	return push_data_common(device_data, size, image_plane_tag, parameter_slot, true);
}

uint32_t beamformer_hip_push_data_burst_with_compute(const void *data, uint32_t frame_size, uint32_t frame_count,
                                                     uint32_t image_plane_tag, uint32_t parameter_slot)
{
	return push_burst_common(data, frame_size, frame_count, image_plane_tag, parameter_slot, false);
}

uint32_t beamformer_hip_push_device_data_burst_with_compute(const void *device_data, uint32_t frame_size, uint32_t frame_count,
                                                            uint32_t image_plane_tag, uint32_t parameter_slot)
{
	return push_burst_common(device_data, frame_size, frame_count, image_plane_tag, parameter_slot, true);
}

/* beamformer_hip_describe_burst, and -- readi_sweep -- beamformer_hip_describe_readi_sweep once the block and the list have passed */
static uint32_t describe_burst_route(uint32_t parameter_slot, uint32_t frame_count, BeamformerHipBurstDescription *out, bool readi_sweep)
{
	Context &c = ctx();
	const ParameterBlock &pb = c.blocks[parameter_slot];
	Plan plan;
	if (!resolved_plan(pb, plan)) return 0;
	uint32_t zfirst, zcount;
	shard_planes(pb, plan, zfirst, zcount);
	const std::vector<BfTransmit> transmits = build_transmit_table(pb);
	std::vector<DasDecision> parts;
	if (plan.das_index >= 0) decide_das_parts(pb, plan, transmits, zfirst, zcount, c.das_path_mode, parts);
	BurstDecision route;
	decide_burst(pb, plan, transmits, parts, zfirst, zcount, c.das_path_mode, frame_count, route, readi_sweep);
	describe_burst_decision(route, out);
	return 1;
}

uint32_t beamformer_hip_describe_burst(uint32_t parameter_slot, uint32_t frame_count, BeamformerHipBurstDescription *out)
{
	if (!valid_parameter_block(parameter_slot) || !check(out != nullptr && frame_count != 0, BeamformerLibErrorKind_InvalidAccess)) return 0;
	return describe_burst_route(parameter_slot, frame_count, out, false);
}

uint32_t beamformer_hip_push_data_readi_sweep_with_compute(const void *data, uint32_t frame_size, uint32_t frame_count,
                                                           const uint32_t *readi_groups, uint32_t image_plane_tag, uint32_t parameter_slot)
{
	return push_readi_sweep_common(data, frame_size, frame_count, readi_groups, image_plane_tag, parameter_slot, false);
}

uint32_t beamformer_hip_push_device_data_readi_sweep_with_compute(const void *device_data, uint32_t frame_size, uint32_t frame_count,
                                                                  const uint32_t *readi_groups, uint32_t image_plane_tag, uint32_t parameter_slot)
{
	return push_readi_sweep_common(device_data, frame_size, frame_count, readi_groups, image_plane_tag, parameter_slot, true);
}

uint32_t beamformer_hip_describe_readi_sweep(uint32_t parameter_slot, const uint32_t *readi_groups, uint32_t frame_count,
                                             BeamformerHipBurstDescription *out)
{
	if (!check(out != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	std::vector<uint32_t> ids;
	if (!resolve_readi_groups(parameter_slot, readi_groups, frame_count, ids)) return 0;
	return describe_burst_route(parameter_slot, frame_count, out, true);
}

uint32_t beamformer_hip_resolve_readi_groups(uint32_t parameter_slot, const uint32_t *readi_groups, uint32_t frame_count, uint32_t *out)
{
	if (!check(out != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	std::vector<uint32_t> ids;
	if (!resolve_readi_groups(parameter_slot, readi_groups, frame_count, ids)) return 0;
	std::memcpy(out, ids.data(), sizeof(uint32_t) * frame_count);
	return 1;
}

uint32_t beamformer_hip_push_data_readi_image_with_compute(const void *data, uint32_t frame_size, uint32_t frame_count,
                                                           const uint32_t *readi_groups, uint32_t image_plane_tag, uint32_t parameter_slot)
{
	return push_readi_image_common(data, frame_size, frame_count, readi_groups, image_plane_tag, parameter_slot, false);
}

uint32_t beamformer_hip_push_device_data_readi_image_with_compute(const void *device_data, uint32_t frame_size, uint32_t frame_count,
                                                                  const uint32_t *readi_groups, uint32_t image_plane_tag, uint32_t parameter_slot)
{
	return push_readi_image_common(device_data, frame_size, frame_count, readi_groups, image_plane_tag, parameter_slot, true);
}

uint32_t beamformer_hip_describe_readi_image(uint32_t parameter_slot, const uint32_t *readi_groups, uint32_t frame_count,
                                             BeamformerHipReadiImageDescription *out)
{
	if (!check(out != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	Context &c = ctx();
	std::vector<uint32_t> ids;
	ParameterBlock derived;
	Plan derived_plan;
	if (!resolve_readi_image(parameter_slot, readi_groups, frame_count, ids, derived, derived_plan)) return 0;
	const ParameterBlock &pb = c.blocks[parameter_slot];
	uint32_t zfirst, zcount;
	shard_planes(pb, derived_plan, zfirst, zcount);
	std::vector<DasDecision> parts;
	if (derived_plan.das_index >= 0 && zcount) decide_das_parts(derived, derived_plan, build_transmit_table(derived), zfirst, zcount, c.das_path_mode, parts);
	ReadiImageDecision route;
	decide_readi_image(derived_plan, parts, pb.parameters.readi_group_count, frame_count, route);
	describe_readi_image_decision(route, out);
	return 1;
}

uint32_t beamformer_hip_get_last_readi_image_info(BeamformerHipReadiImageInfo *out)
{
	if (!check(out != nullptr, BeamformerLibErrorKind_InvalidAccess) || !ensure_device()) return 0;
	return last_readi_image_info(out);
}

uint32_t beamformer_hip_get_last_burst_info(BeamformerHipBurstInfo *out)
{
	if (!check(out != nullptr, BeamformerLibErrorKind_InvalidAccess) || !ensure_device()) return 0;
	return last_burst_info(out);
}

uint32_t beamformer_hip_push_data_views_with_compute(const void *data, uint32_t size, const BeamformerHipView *views, uint32_t view_count,
                                                     uint32_t parameter_slot)
{
	return push_views_common(data, size, views, view_count, parameter_slot, false);
}

uint32_t beamformer_hip_push_device_data_views_with_compute(const void *device_data, uint32_t size, const BeamformerHipView *views, uint32_t view_count,
                                                            uint32_t parameter_slot)
{
	return push_views_common(device_data, size, views, view_count, parameter_slot, true);
}

uint32_t beamformer_hip_describe_views(uint32_t parameter_slot, const BeamformerHipView *views, uint32_t view_count, BeamformerHipViewsDescription *out)
{
	if (!check(out != nullptr, BeamformerLibErrorKind_InvalidAccess) || !validate_views(views, view_count, parameter_slot)) return 0;
	Context &c = ctx();
	const ParameterBlock &pb = c.blocks[parameter_slot];
	Plan plan;
	if (!resolved_plan(pb, plan)) return 0;
	ViewsDecision route;
	decide_views(pb, plan, build_transmit_table(pb), view_grids(views, view_count).data(), view_count, c.das_path_mode, route);
	describe_views_decision(route, view_count, out);
	return 1;
}

uint32_t beamformer_hip_get_last_views_info(BeamformerHipViewsInfo *out)
{
	if (!check(out != nullptr, BeamformerLibErrorKind_InvalidAccess) || !ensure_device()) return 0;
	return last_views_info(out);
}

uint32_t beamformer_hip_push_data_burst_views_with_compute(const void *data, uint32_t frame_size, uint32_t frame_count, const BeamformerHipView *views,
                                                           uint32_t view_count, uint32_t parameter_slot)
{
	return push_burst_views_common(data, frame_size, frame_count, views, view_count, parameter_slot, false);
}

uint32_t beamformer_hip_push_device_data_burst_views_with_compute(const void *device_data, uint32_t frame_size, uint32_t frame_count,
                                                                  const BeamformerHipView *views, uint32_t view_count, uint32_t parameter_slot)
{
	return push_burst_views_common(device_data, frame_size, frame_count, views, view_count, parameter_slot, true);
}

uint32_t beamformer_hip_describe_burst_views(uint32_t parameter_slot, uint32_t frame_count, const BeamformerHipView *views, uint32_t view_count,
                                             BeamformerHipBurstViewsDescription *out)
{
	if (!check(out != nullptr, BeamformerLibErrorKind_InvalidAccess) || !validate_burst_views(frame_count, views, view_count, parameter_slot)) return 0;
	Context &c = ctx();
	const ParameterBlock &pb = c.blocks[parameter_slot];
	Plan plan;
	if (!resolved_plan(pb, plan)) return 0;
	BurstViewsDecision route;
	decide_burst_views(pb, plan, build_transmit_table(pb), view_grids(views, view_count).data(), view_count, c.das_path_mode, frame_count, route);
	describe_burst_views_decision(route, view_count, out);
	return 1;
}

uint32_t beamformer_hip_get_last_burst_views_info(BeamformerHipBurstViewsInfo *out)
{
	if (!check(out != nullptr, BeamformerLibErrorKind_InvalidAccess) || !ensure_device()) return 0;
	return last_burst_views_info(out);
}

uint32_t beamformer_hip_push_data_variants_with_compute(const void *data, uint32_t size, const BeamformerHipDasVariant *variants, uint32_t variant_count,
                                                        uint32_t image_plane_tag, uint32_t parameter_slot)
{
	return push_variants_common(data, size, variants, variant_count, image_plane_tag, parameter_slot, false);
}

uint32_t beamformer_hip_push_device_data_variants_with_compute(const void *device_data, uint32_t size, const BeamformerHipDasVariant *variants,
                                                               uint32_t variant_count, uint32_t image_plane_tag, uint32_t parameter_slot)
{
	return push_variants_common(device_data, size, variants, variant_count, image_plane_tag, parameter_slot, true);
}

uint32_t beamformer_hip_describe_variants(uint32_t parameter_slot, const BeamformerHipDasVariant *variants, uint32_t variant_count,
                                          BeamformerHipVariantsDescription *out)
{
	if (!check(out != nullptr, BeamformerLibErrorKind_InvalidAccess) || !validate_variants(variants, variant_count, parameter_slot)) return 0;
	Context &c = ctx();
	const ParameterBlock &pb = c.blocks[parameter_slot];
	Plan plan;
	if (!resolved_plan(pb, plan)) return 0;
	VariantsDecision route;
	decide_variants(pb, plan, build_transmit_table(pb), das_variants(variants, variant_count).data(), variant_count, c.das_path_mode, route);
	describe_variants_decision(route, variant_count, out);
	return 1;
}

uint32_t beamformer_hip_get_last_variants_info(BeamformerHipVariantsInfo *out)
{
	if (!check(out != nullptr, BeamformerLibErrorKind_InvalidAccess) || !ensure_device()) return 0;
	return last_variants_info(out);
}

uint32_t beamformer_hip_synchronize(void)
{
	if (!ensure_device()) return 0;
	return wait_for_frames(-1);
}

uint32_t beamformer_hip_get_last_frame_info(BeamformerHipFrameInfo *out)
{
	Context &c = ctx();
	const Device &d = c.devices[0];      /* with several devices: the ingest device's slab */
	const FrameRecord *newest = c.device_ready ? newest_record(d) : nullptr;      /* null after a push that did not complete */
	if (!check(newest != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	const FrameRecord &f = *newest;
	out->device_pointer = (char *)d.ring.ptr + f.offset;
	out->size_bytes = f.bytes;
	out->points[0] = f.points[0]; out->points[1] = f.points[1]; out->points[2] = f.points[2];
	out->data_kind = (uint32_t)f.data_kind;
	out->frame_id = f.id; out->parameter_block = f.block;
	return 1;
}

uint32_t beamformer_hip_get_last_frame_timings(BeamformerHipFrameTimings *out)
{
	if (!ensure_device()) return 0;
	return last_frame_timings(out);
}

uint32_t beamformer_hip_enable_frame_graphs(uint32_t enable) { ctx().frame_graphs = enable != 0; return 1; }

uint32_t beamformer_hip_frame_graph_counts(uint64_t *frames_replayed, uint64_t *graphs_instantiated)
{
	if (frames_replayed)     *frames_replayed     = ctx().graph_frames;
	if (graphs_instantiated) *graphs_instantiated = ctx().graph_instantiations;
	return 1;
}

uint32_t beamformer_hip_enable_pair_counting(uint32_t enable) { ctx().count_pairs = enable != 0; return 1; }

uint32_t beamformer_hip_frame_min_max(float out_min_max[2])
{
	if (!ensure_device()) return 0;
	return frame_min_max(out_min_max);
}

uint32_t beamformer_hip_copy_das_input(void *out, uint64_t size)
{
	if (!out) return set_error(BeamformerLibErrorKind_InvalidAccess);
	return copy_das_input(out, size);
}

uint32_t beamformer_hip_copy_das_input_frame(uint32_t frame, void *out, uint64_t size)
{
	if (!out) return set_error(BeamformerLibErrorKind_InvalidAccess);
	return copy_das_input_frame(frame, out, size);
}

uint32_t beamformer_hip_sum_last_frames(uint32_t count, void *out, uint64_t out_size)
{
	if (!out) return set_error(BeamformerLibErrorKind_InvalidAccess);
	if (!ensure_device()) return 0;
	return sum_last_frames(count, out, out_size);
}

/* the three below serve frames that exist: they start no device (no device yet: there is no frame, InvalidAccess) */
uint32_t beamformer_hip_score_last_frames(uint32_t count, const BeamformerHipFrameRegion *region, BeamformerHipFrameMetrics *out, float *device_ms)
{
	if (!check(count >= 1 && count <= BEAMFORMER_HIP_MAX_SCORED_FRAMES, BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check(out != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	return score_last_frames(count, region, out, device_ms);
}

/* The arguments the five peak calls share, refused in the one order all five keep -- with several faults at once the order decides which
 * error kind the caller sees: the ranges (BufferOverflow), then the pointers, the counts and the values (InvalidAccess).  capped,
 * placed: the call has a max_per_frame, placements; linking: it links frames -- two at the least, within a max_distance; min_length:
 * null where the call has none; outputs: the call's own output pointers are all there.  A call's further checks come behind these. */
static bool valid_peak_query(const PeakQuery &q, bool capped, bool placed, bool linking, const uint32_t *min_length, bool outputs)
{
	if (!check(q.count >= (linking ? 2u : 1u) && q.count <= BEAMFORMER_HIP_MAX_SCORED_FRAMES, BeamformerLibErrorKind_BufferOverflow)) return false;
	if (capped && !check(q.max_per_frame >= 1 && q.max_per_frame <= BEAMFORMER_HIP_MAX_PEAKS_PER_FRAME, BeamformerLibErrorKind_BufferOverflow)) return false;
	if (min_length && !check(*min_length >= 1 && *min_length <= BEAMFORMER_HIP_MAX_SCORED_FRAMES, BeamformerLibErrorKind_BufferOverflow)) return false;
	if (!check(outputs && q.thresholds != nullptr && (!placed || q.placements != nullptr), BeamformerLibErrorKind_InvalidAccess)) return false;
	if (!check(q.threshold_count == 1 || q.threshold_count == q.count, BeamformerLibErrorKind_InvalidAccess)) return false;
	if (placed && !check(q.placement_count == 1 || q.placement_count == q.count, BeamformerLibErrorKind_InvalidAccess)) return false;
	for (uint32_t k = 0; k < q.threshold_count; k++)
		if (!check(std::isfinite(q.thresholds[k]) && q.thresholds[k] >= 0.0f, BeamformerLibErrorKind_InvalidAccess)) return false;
	for (size_t k = 0; placed && k < (size_t)12 * q.placement_count; k++)
		if (!check(std::isfinite(q.placements[k]), BeamformerLibErrorKind_InvalidAccess)) return false;
	return !linking || check(q.max_distance >= 0.0f && q.max_distance <= BEAMFORMER_HIP_MAX_PAIR_DISTANCE, BeamformerLibErrorKind_InvalidAccess);   /* (a NaN fails both) */
}

uint32_t beamformer_hip_find_peaks_last_frames(uint32_t count, const BeamformerHipFrameRegion *region, const float *thresholds, uint32_t threshold_count,
                                               uint32_t max_per_frame, BeamformerHipFramePeaks *frames, BeamformerHipFramePeak *peaks,
                                               uint32_t *peak_count, float *device_ms)
{
	const PeakQuery q{count, region, thresholds, threshold_count, nullptr, 0, 0, 0.0f, max_per_frame};
	if (!valid_peak_query(q, true, false, false, nullptr, frames != nullptr && peaks != nullptr && peak_count != nullptr)) return 0;
	return find_peaks_last_frames(q, frames, peaks, peak_count, device_ms);
}

uint32_t beamformer_hip_quantiles_last_frames(uint32_t count, const BeamformerHipFrameRegion *region, const double *fractions, uint32_t fraction_count,
                                              BeamformerHipFrameQuantiles *frames, BeamformerHipFrameQuantile *quantiles, uint32_t *histograms,
                                              float *device_ms)
{
	if (!check(count >= 1 && count <= BEAMFORMER_HIP_MAX_SCORED_FRAMES, BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check(fraction_count >= 1 && fraction_count <= BEAMFORMER_HIP_MAX_QUANTILES, BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check(fractions != nullptr && frames != nullptr && quantiles != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	for (uint32_t k = 0; k < fraction_count; k++)
		if (!check(fractions[k] >= 0.0 && fractions[k] <= 1.0, BeamformerLibErrorKind_InvalidAccess)) return 0;      /* (a NaN fails both) */
	return quantiles_last_frames(count, region, fractions, fraction_count, frames, quantiles, histograms, device_ms);
}

/* host only: the threshold of the peak calls that goes with a decision value (include/ogl_beamformer_hip.h has the rule) */
uint32_t beamformer_hip_peak_threshold_of(float decision_value, uint32_t data_kind, float *threshold)
{
	if (!check(threshold != nullptr && std::isfinite(decision_value) && decision_value >= 0.0f, BeamformerLibErrorKind_InvalidAccess)) return 0;
	if (!check(data_kind == BeamformerDataKind_Float32 || data_kind == BeamformerDataKind_Float32Complex, BeamformerLibErrorKind_InvalidAccess)) return 0;
	*threshold = peak_threshold_of(decision_value, data_kind == BeamformerDataKind_Float32Complex);
	return 1;
}

/* host only: one view a peak, a patch around it (include/ogl_beamformer_hip.h has the algebra) */
uint32_t beamformer_hip_peaks_to_views(const float source_voxel_transform[16], const uint32_t source_points[3], const BeamformerHipFramePeak *peaks,
                                       uint32_t peak_count, const uint32_t patch_points[3], const float patch_extent_voxels[3], uint32_t use_offsets,
                                       uint32_t image_plane_tag, BeamformerHipView *out)
{
	if (!check(source_voxel_transform && source_points && peaks && patch_points && patch_extent_voxels && out, BeamformerLibErrorKind_InvalidAccess)) return 0;
	for (int a = 0; a < 3; a++)
		if (!check(patch_points[a] != 0 && std::isfinite(patch_extent_voxels[a]) && patch_extent_voxels[a] >= 0.0f, BeamformerLibErrorKind_InvalidAccess)) return 0;
	const float *m = source_voxel_transform;          /* column major: m[4 * column + row] */
	for (uint32_t n = 0; n < peak_count; n++) {
		const BeamformerHipFramePeak &p = peaks[n];
		BeamformerHipView &v = out[n];
		double origin[3], scale[3];
		for (int a = 0; a < 3; a++) {
			const double last = source_points[a] > 1 ? (double)source_points[a] - 1.0 : 1.0;
			const double c = ((double)p.index[a] + (use_offsets ? (double)p.offset[a] : 0.0)) / last, s = (double)patch_extent_voxels[a] / last;
			const bool spans = patch_points[a] > 1;
			origin[a] = spans ? c - 0.5 * s : c;
			scale[a]  = spans ? s : 1.0;
		}
		for (int row = 0; row < 4; row++) {
			for (int a = 0; a < 3; a++) v.das_voxel_transform[4 * a + row] = (float)((double)m[4 * a + row] * scale[a]);
			v.das_voxel_transform[12 + row] = (float)((double)m[row] * origin[0] + (double)m[4 + row] * origin[1] + (double)m[8 + row] * origin[2] + (double)m[12 + row]);
		}
		for (int a = 0; a < 3; a++) v.output_points[a] = patch_points[a];
		v.image_plane_tag = image_plane_tag;
	}
	return 1;
}

/* a map's extents against its voxel limit, the device started, the map (re)allocated; points null: released, with no device needed */
static uint32_t reset_deposit_map(FrameOps::DepositMap &map, const uint32_t points[3], uint64_t max_voxels)
{
	if (!points) return deposit_map_reset(map, nullptr);
	if (!check(points[0] && points[1] && points[2], BeamformerLibErrorKind_InvalidAccess)) return 0;
	if (!check((uint64_t)points[0] * points[1] <= max_voxels && (uint64_t)points[0] * points[1] * points[2] <= max_voxels,
	           BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!ensure_device()) return 0;
	return deposit_map_reset(map, points);
}

uint32_t beamformer_hip_localisation_map_reset(const uint32_t points[3])
{
	return reset_deposit_map(ctx().devices[0].ops.map, points, BEAMFORMER_HIP_MAX_MAP_VOXELS);
}

/* (serves frames that exist, as the calls above: it starts no device) */
uint32_t beamformer_hip_accumulate_peaks_last_frames(uint32_t count, const BeamformerHipFrameRegion *region, const float *thresholds,
                                                     uint32_t threshold_count, const double *placements, uint32_t placement_count,
                                                     uint32_t use_offsets, BeamformerHipMapDeposits *frames, float *device_ms)
{
	const PeakQuery q{count, region, thresholds, threshold_count, placements, placement_count, use_offsets, 0.0f, 0};
	if (!valid_peak_query(q, false, true, false, nullptr, true)) return 0;
	return accumulate_peaks_last_frames(q, frames, device_ms);
}

uint32_t beamformer_hip_localisation_map_copy(uint32_t *out, uint64_t out_count, BeamformerHipMapInfo *info)
{
	if (!check(out != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	return localisation_map_copy(out, out_count, info);
}

uint32_t beamformer_hip_queue_localisation_map(float scale, uint32_t image_plane_tag, uint32_t *frame_id, float *device_ms)
{
	if (!check(std::isfinite(scale), BeamformerLibErrorKind_InvalidAccess)) return 0;
	return queue_localisation_map(scale, image_plane_tag, frame_id, device_ms);
}

uint32_t beamformer_hip_track_map_reset(const uint32_t points[3])
{
	return reset_deposit_map(ctx().devices[0].ops.tracks, points, BEAMFORMER_HIP_MAX_TRACK_MAP_VOXELS);
}

/* (the three below serve frames that exist, as the calls above: they start no device) */
uint32_t beamformer_hip_pair_peaks_last_frames(uint32_t count, const BeamformerHipFrameRegion *region, const float *thresholds,
                                               uint32_t threshold_count, const double *placements, uint32_t placement_count,
                                               uint32_t use_offsets, float max_distance, uint32_t max_per_frame, uint32_t deposit,
                                               BeamformerHipPeakPairs *rows, BeamformerHipPeakPair *pairs, uint32_t *pair_count, float *device_ms)
{
	const PeakQuery q{count, region, thresholds, threshold_count, placements, placement_count, use_offsets, max_distance, max_per_frame};
	if (!valid_peak_query(q, true, true, true, nullptr, rows != nullptr && pair_count != nullptr)) return 0;
	return pair_peaks_last_frames(q, deposit, rows, pairs, pair_count, device_ms);
}

static bool valid_track_deposit(uint32_t deposit)
{
	return check((deposit & ~(BEAMFORMER_HIP_TRACK_DEPOSIT_POINTS | BEAMFORMER_HIP_TRACK_DEPOSIT_LINKS)) == 0, BeamformerLibErrorKind_InvalidAccess);
}

uint32_t beamformer_hip_track_peaks_last_frames(uint32_t count, const BeamformerHipFrameRegion *region, const float *thresholds,
                                                uint32_t threshold_count, const double *placements, uint32_t placement_count,
                                                uint32_t use_offsets, float max_distance, uint32_t max_per_frame, uint32_t min_length,
                                                uint32_t deposit, BeamformerHipTrackedFrame *rows, BeamformerHipPeakTrack *tracks,
                                                BeamformerHipTrackPoint *points, uint32_t *track_count, uint32_t *point_count, float *device_ms)
{
	const PeakQuery q{count, region, thresholds, threshold_count, placements, placement_count, use_offsets, max_distance, max_per_frame};
	if (!valid_peak_query(q, true, true, true, &min_length, rows != nullptr && track_count != nullptr && point_count != nullptr)) return 0;
	if (!valid_track_deposit(deposit)) return 0;
	return track_peaks_last_frames(q, min_length, deposit, rows, tracks, points, track_count, point_count, device_ms);
}

uint32_t beamformer_hip_draw_tracks_last_frames(uint32_t count, const BeamformerHipFrameRegion *region, const float *thresholds,
                                                uint32_t threshold_count, const double *placements, uint32_t placement_count,
                                                uint32_t use_offsets, float max_distance, uint32_t max_per_frame, uint32_t min_length,
                                                uint32_t smooth, uint32_t deposit, BeamformerHipDrawnFrame *rows, float *device_ms)
{
	const PeakQuery q{count, region, thresholds, threshold_count, placements, placement_count, use_offsets, max_distance, max_per_frame};
	if (!valid_peak_query(q, true, true, true, &min_length, rows != nullptr)) return 0;
	if (!valid_track_deposit(deposit)) return 0;
	if (!check(smooth <= BEAMFORMER_HIP_MAX_TRACK_SMOOTH, BeamformerLibErrorKind_BufferOverflow)) return 0;      /* (behind every InvalidAccess) */
	return draw_tracks_last_frames(q, min_length, smooth, deposit, rows, device_ms);
}

uint32_t beamformer_hip_track_map_copy(uint32_t *counts, int64_t *sums, uint64_t out_count, BeamformerHipTrackMapInfo *info)
{
	if (!check(counts != nullptr && sums != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	return track_map_copy(counts, sums, out_count, info);
}

uint32_t beamformer_hip_queue_track_map(uint32_t component, float scale, uint32_t min_pairs, uint32_t image_plane_tag, uint32_t *frame_id, float *device_ms)
{
	if (!check(component < BEAMFORMER_HIP_TRACK_MAP_COMPONENTS && std::isfinite(scale), BeamformerLibErrorKind_InvalidAccess)) return 0;
	return queue_track_map(component, scale, min_pairs, image_plane_tag, frame_id, device_ms);
}

/* host only: S_map^-1 M_map^-1 M_frame S_frame in double (include/ogl_beamformer_hip.h has the algebra) */
uint32_t beamformer_hip_map_placement(const float frame_voxel_transform[16], const uint32_t frame_points[3], const float map_voxel_transform[16],
                                      const uint32_t map_points[3], double out[12])
{
	if (!check(frame_voxel_transform && frame_points && map_voxel_transform && map_points && out, BeamformerLibErrorKind_InvalidAccess)) return 0;
	for (int a = 0; a < 3; a++)
		if (!check(frame_points[a] != 0 && map_points[a] != 0, BeamformerLibErrorKind_InvalidAccess)) return 0;
	const float *f = frame_voxel_transform, *g = map_voxel_transform;      /* column major: m[4 * column + row] */
	/* the map's linear part L (rows r, columns c) and its cofactor inverse */
	double L[3][3], norms = 1.0;
	for (int col = 0; col < 3; col++) {
		double n2 = 0.0;
		for (int r = 0; r < 3; r++) { L[r][col] = (double)g[4 * col + r]; n2 += L[r][col] * L[r][col]; }
		norms *= std::sqrt(n2);
	}
	const double c00 = L[1][1] * L[2][2] - L[1][2] * L[2][1], c01 = L[1][2] * L[2][0] - L[1][0] * L[2][2], c02 = L[1][0] * L[2][1] - L[1][1] * L[2][0];
	const double det = L[0][0] * c00 + L[0][1] * c01 + L[0][2] * c02;
	/* singular: a determinant that is not finite, or not above 10^-12 of the product of the columns' lengths (float32 columns closer to
	 * a common plane than that span no volume their own precision could tell from none) */
	if (!check(std::isfinite(det) && std::fabs(det) > 1e-12 * norms, BeamformerLibErrorKind_InvalidAccess)) return 0;
	const double inv[3][3] = {
		{c00 / det, (L[0][2] * L[2][1] - L[0][1] * L[2][2]) / det, (L[0][1] * L[1][2] - L[0][2] * L[1][1]) / det},
		{c01 / det, (L[0][0] * L[2][2] - L[0][2] * L[2][0]) / det, (L[0][2] * L[1][0] - L[0][0] * L[1][2]) / det},
		{c02 / det, (L[0][1] * L[2][0] - L[0][0] * L[2][1]) / det, (L[0][0] * L[1][1] - L[0][1] * L[1][0]) / det}};
	double result[12];
	for (int r = 0; r < 3; r++) {
		const double map_last = map_points[r] > 1 ? (double)map_points[r] - 1.0 : 1.0;        /* S_map^-1 */
		for (int col = 0; col < 4; col++) {
			/* column col of M_frame S_frame; the last one: the frames' origin seen from the map's */
			const double frame_last = col < 3 && frame_points[col] > 1 ? (double)frame_points[col] - 1.0 : 1.0;
			double v[3];
			for (int k = 0; k < 3; k++) v[k] = col < 3 ? (double)f[4 * col + k] / frame_last : (double)f[12 + k] - (double)g[12 + k];
			result[4 * r + col] = (inv[r][0] * v[0] + inv[r][1] * v[1] + inv[r][2] * v[2]) * map_last;
		}
	}
	for (int k = 0; k < 12; k++)
		if (!check(std::isfinite(result[k]), BeamformerLibErrorKind_InvalidAccess)) return 0;
	std::memcpy(out, result, sizeof(result));
	return 1;
}

uint32_t beamformer_hip_gram_last_frames(uint32_t count, const BeamformerHipFrameRegion *region, double *gram, BeamformerHipEnsembleInfo *info,
                                         float *device_ms)
{
	if (!check(count >= 1 && count <= BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES, BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check(gram != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	return gram_last_frames(count, region, gram, info, device_ms);
}

/* host only: the Jacobi eigendecomposition and the projector are host_math.cpp's */
uint32_t beamformer_hip_clutter_projector(const double *gram, uint32_t count, uint32_t remove_high, uint32_t remove_low, float *weights,
                                          double *eigenvalues)
{
	if (!check(count >= 1 && count <= BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES, BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check(gram != nullptr && weights != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	if (!check((uint64_t)remove_high + remove_low <= count, BeamformerLibErrorKind_InvalidAccess)) return 0;
	return check(clutter_projector(gram, count, remove_high, remove_low, weights, eigenvalues), BeamformerLibErrorKind_InvalidAccess) ? 1 : 0;
}

uint32_t beamformer_hip_mix_last_frames(uint32_t count, const float *weights, uint32_t out_count, uint32_t image_plane_tag, uint32_t *first_frame_id,
                                        float *device_ms)
{
	if (!check(count >= 1 && count <= BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES && out_count >= 1 && out_count <= BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES,
	           BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check(weights != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	for (size_t n = 0; n < (size_t)2 * count * out_count; n++)
		if (!check(std::isfinite(weights[n]), BeamformerLibErrorKind_InvalidAccess)) return 0;
	return mix_last_frames(count, weights, out_count, image_plane_tag, first_frame_id, device_ms);
}

uint32_t beamformer_hip_gram_boxes_last_frames(uint32_t count, const BeamformerHipFrameRegion *regions, uint32_t region_count, double *grams,
                                               BeamformerHipEnsembleInfo *infos, float *device_ms)
{
	if (!check(count >= 1 && count <= BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES, BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check(region_count >= 1 && region_count <= BEAMFORMER_HIP_MAX_GRAM_BOXES, BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check((uint64_t)region_count * count * count <= BEAMFORMER_HIP_MAX_GRAM_BOX_ENTRIES, BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check(grams != nullptr && regions != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	return gram_boxes_last_frames(count, regions, region_count, grams, infos, device_ms);
}

/* host only: the boxes of a lattice's nodes, clipped to the frame (include/ogl_beamformer_hip.h has the rule) */
uint32_t beamformer_hip_lattice_boxes(const uint32_t points[3], const uint32_t nodes[3], const uint32_t node_first[3], const uint32_t node_step[3],
                                      const uint32_t half[3], BeamformerHipFrameRegion *regions)
{
	if (!check(points && nodes && node_first && node_step && half && regions, BeamformerLibErrorKind_InvalidAccess)) return 0;
	uint64_t node_product = 1;
	for (int a = 0; a < 3; a++) {
		if (!check(points[a] != 0 && nodes[a] != 0, BeamformerLibErrorKind_InvalidAccess)) return 0;
		node_product *= nodes[a];                             /* (at most 1024 x 2^32 - 1: no overflow) */
		if (!check(node_product <= BEAMFORMER_HIP_MAX_MIX_NODES, BeamformerLibErrorKind_BufferOverflow)) return 0;
	}
	/* an axis's boxes: [max(0, P - half), min(points, P + half + 1)), P in 64 bits */
	std::vector<uint32_t> first[3], count[3];
	for (int a = 0; a < 3; a++) {
		if (!check(nodes[a] == 1 || node_step[a] != 0, BeamformerLibErrorKind_InvalidAccess)) return 0;
		for (uint32_t j = 0; j < nodes[a]; j++) {
			const uint64_t at = (uint64_t)node_first[a] + (uint64_t)j * (nodes[a] > 1 ? node_step[a] : 0u);
			const uint64_t lo = at > half[a] ? at - half[a] : 0, hi = at + half[a] + 1u < points[a] ? at + half[a] + 1u : points[a];
			if (!check(lo < hi, BeamformerLibErrorKind_InvalidAccess)) return 0;      /* the box misses the frame */
			first[a].push_back((uint32_t)lo); count[a].push_back((uint32_t)(hi - lo));
		}
	}
	for (uint32_t jz = 0; jz < nodes[2]; jz++)
		for (uint32_t jy = 0; jy < nodes[1]; jy++)
			for (uint32_t jx = 0; jx < nodes[0]; jx++) {
				BeamformerHipFrameRegion &r = regions[((size_t)jz * nodes[1] + jy) * nodes[0] + jx];
				const uint32_t j[3] = {jx, jy, jz};
				for (int a = 0; a < 3; a++) { r.first[a] = first[a][j[a]]; r.count[a] = count[a][j[a]]; }
			}
	return 1;
}

uint32_t beamformer_hip_mix_field_last_frames(uint32_t count, const float *weights, const uint32_t nodes[3], const uint32_t node_first[3],
                                              const uint32_t node_step[3], uint32_t out_count, uint32_t image_plane_tag, uint32_t *first_frame_id,
                                              float *device_ms)
{
	if (!check(count >= 1 && count <= BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES && out_count >= 1 && out_count <= BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES,
	           BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check(weights != nullptr && nodes != nullptr && node_first != nullptr && node_step != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	uint64_t node_product = 1;
	for (int a = 0; a < 3; a++) {
		if (!check(nodes[a] >= 1, BeamformerLibErrorKind_BufferOverflow)) return 0;
		node_product *= nodes[a];                             /* (at most 1024 x 2^32 - 1: no overflow) */
		if (!check(node_product <= BEAMFORMER_HIP_MAX_MIX_NODES, BeamformerLibErrorKind_BufferOverflow)) return 0;
	}
	if (!check(node_product * out_count * count <= BEAMFORMER_HIP_MAX_MIX_FIELD_ENTRIES, BeamformerLibErrorKind_BufferOverflow)) return 0;
	for (int a = 0; a < 3; a++)
		if (!check(nodes[a] == 1 || node_step[a] != 0, BeamformerLibErrorKind_InvalidAccess)) return 0;
	for (size_t n = 0; n < (size_t)2 * node_product * out_count * count; n++)
		if (!check(std::isfinite(weights[n]), BeamformerLibErrorKind_InvalidAccess)) return 0;
	return mix_field_last_frames(count, weights, nodes, node_first, node_step, out_count, image_plane_tag, first_frame_id, device_ms);
}

uint32_t beamformer_hip_autocorrelate_last_frames(uint32_t count, const float *weights, uint32_t rows, uint32_t lag_count, uint32_t image_plane_tag,
                                                  uint32_t *first_frame_id, float *device_ms)
{
	if (!check(count >= 1 && count <= BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES && rows >= 1 && rows <= BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES,
	           BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check(lag_count >= 1 && lag_count <= BEAMFORMER_HIP_MAX_LAGS && lag_count <= rows, BeamformerLibErrorKind_InvalidAccess)) return 0;
	if (!check(weights != nullptr || rows == count, BeamformerLibErrorKind_InvalidAccess)) return 0;
	for (size_t n = 0; weights && n < (size_t)2 * count * rows; n++)
		if (!check(std::isfinite(weights[n]), BeamformerLibErrorKind_InvalidAccess)) return 0;
	return autocorrelate_last_frames(count, weights, rows, lag_count, image_plane_tag, first_frame_id, device_ms);
}

uint32_t beamformer_hip_convolve_last_frames(uint32_t count, const float *const taps[3], const uint32_t tap_counts[3], uint32_t mode,
                                             uint32_t image_plane_tag, uint32_t *first_frame_id, float *device_ms)
{
	if (!check(count >= 1 && count <= BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES, BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check(taps != nullptr && tap_counts != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	for (int a = 0; a < 3; a++)
		if (!check(tap_counts[a] <= BEAMFORMER_HIP_MAX_SPATIAL_TAPS, BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check(mode < BeamformerHipSpatialMode_Count && (tap_counts[0] | tap_counts[1] | tap_counts[2]) != 0, BeamformerLibErrorKind_InvalidAccess)) return 0;
	for (int a = 0; a < 3; a++) {
		if (tap_counts[a] == 0) continue;
		if (!check(tap_counts[a] % 2u == 1u && taps[a] != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
		for (uint32_t t = 0; t < tap_counts[a]; t++) {
			const float h = taps[a][t];
			if (!check(std::isfinite(h) && !(mode == BeamformerHipSpatialMode_Normalised && h < 0.0f), BeamformerLibErrorKind_InvalidAccess)) return 0;
		}
	}
	return convolve_last_frames(count, taps, tap_counts, mode, image_plane_tag, first_frame_id, device_ms);
}

uint32_t beamformer_hip_correlate_last_frames(uint32_t count, uint32_t reference, const BeamformerHipFrameRegion *regions, uint32_t region_count,
                                              const uint32_t max_shift[3], BeamformerHipShiftCorrelation *table, BeamformerHipCorrelationInfo *info,
                                              float *device_ms)
{
	if (!check(count >= 1 && count <= BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES, BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check(!regions || (region_count >= 1 && region_count <= BEAMFORMER_HIP_MAX_CORRELATION_REGIONS), BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check(table != nullptr && max_shift != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	uint64_t shifts = 1;
	for (int a = 0; a < 3; a++) {
		if (!check(max_shift[a] <= BEAMFORMER_HIP_MAX_SHIFT, BeamformerLibErrorKind_BufferOverflow)) return 0;
		shifts *= 2u * max_shift[a] + 1u;
	}
	if (!check(shifts <= BEAMFORMER_HIP_MAX_SHIFTS, BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check((uint64_t)(regions ? region_count : 1u) * count * shifts <= BEAMFORMER_HIP_MAX_CORRELATION_ENTRIES, BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check(reference < count, BeamformerLibErrorKind_InvalidAccess)) return 0;
	return correlate_last_frames(count, reference, regions, region_count, max_shift, table, info, device_ms);
}

/* host only: the peak of every table and a parabola through its neighbours along each axis (include/ogl_beamformer_hip.h has the rules) */
uint32_t beamformer_hip_displacements_from_correlation(const BeamformerHipShiftCorrelation *tables, uint32_t table_count, const uint32_t max_shift[3],
                                                       uint32_t normalised, BeamformerHipDisplacement *out)
{
	static_assert(sizeof(BeamformerHipDisplacement) == 40 && sizeof(BeamformerHipShiftCorrelation) == 40, "records without padding");
	if (!check(tables != nullptr && max_shift != nullptr && out != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	if (!check(table_count >= 1, BeamformerLibErrorKind_BufferOverflow)) return 0;
	uint32_t window[3], shifts = 1;
	for (int a = 0; a < 3; a++) {
		if (!check(max_shift[a] <= BEAMFORMER_HIP_MAX_SHIFT, BeamformerLibErrorKind_BufferOverflow)) return 0;
		window[a] = 2u * max_shift[a] + 1u;
		shifts *= window[a];
	}
	if (!check(shifts <= BEAMFORMER_HIP_MAX_SHIFTS, BeamformerLibErrorKind_BufferOverflow)) return 0;
	const uint32_t stride[3] = {1u, window[0], window[0] * window[1]};
	/* an entry's score; negative: no candidate */
	auto score = [normalised](const BeamformerHipShiftCorrelation &e) -> double {
		if (!e.terms || !std::isfinite(e.re) || !std::isfinite(e.im) || !std::isfinite(e.energy_reference) || !std::isfinite(e.energy_frame)) return -1.0;
		const double q = e.re * e.re + e.im * e.im;
		if (!normalised) return q;
		if (!(e.energy_reference > 0.0) || !(e.energy_frame > 0.0)) return -1.0;
		return q / (e.energy_reference * e.energy_frame);
	};
	bool any = false;
	for (uint32_t n = 0; n < table_count; n++) {
		const BeamformerHipShiftCorrelation *t = tables + (size_t)n * shifts;
		BeamformerHipDisplacement &d = out[n];
		std::memset(&d, 0, sizeof(d));
		double   best = -1.0;
		uint32_t best_at = 0;
		for (uint32_t s = 0; s < shifts; s++) {
			const double q = score(t[s]);
			if (q >= 0.0 && q > best) { best = q; best_at = s; }
		}
		if (best < 0.0) continue;
		any = true;
		const BeamformerHipShiftCorrelation &peak = t[best_at];
		const uint32_t index[3] = {best_at % window[0], best_at / window[0] % window[1], best_at / (window[0] * window[1])};
		const double m0 = std::sqrt(best);
		for (int a = 0; a < 3; a++) {
			const int32_t shift = (int32_t)index[a] - (int32_t)max_shift[a];
			double offset = 0.0;
			if (max_shift[a] > 0 && index[a] > 0 && index[a] + 1u < window[a]) {
				const double below = score(t[best_at - stride[a]]), above = score(t[best_at + stride[a]]);
				if (below >= 0.0 && above >= 0.0) {
					const double lo = std::sqrt(below), hi = std::sqrt(above), den = (lo + hi) - (m0 + m0);
					if (den < 0.0) {
						offset = 0.5 * (lo - hi) / den;
						offset = offset < -0.5 ? -0.5 : offset > 0.5 ? 0.5 : offset;
						d.fitted |= 1u << a;
					}
				}
			}
			if (max_shift[a] > 0 && (uint32_t)(shift < 0 ? -shift : shift) == max_shift[a]) d.at_window_edge |= 1u << a;
			d.shift[a] = shift;
			d.displacement[a] = (float)((double)shift + offset);
		}
		const double energy = peak.energy_reference * peak.energy_frame;
		d.coefficient = energy > 0.0 ? (float)(std::sqrt(peak.re * peak.re + peak.im * peak.im) / std::sqrt(energy)) : 0.0f;
		d.phase = (float)std::atan2(peak.im, peak.re);
	}
	return check(any, BeamformerLibErrorKind_InvalidAccess) ? 1 : 0;
}

uint32_t beamformer_hip_warp_last_frames(uint32_t count, const float *field, const uint32_t nodes[3], const float node_first[3],
                                         const float node_step[3], const float *rotations, uint32_t interpolation, uint32_t edge,
                                         uint32_t image_plane_tag, uint32_t *first_frame_id, float *device_ms)
{
	if (!check(count >= 1 && count <= BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES, BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check(field != nullptr && nodes != nullptr && node_first != nullptr && node_step != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	uint64_t node_product = 1;
	for (int a = 0; a < 3; a++) {
		if (!check(nodes[a] >= 1, BeamformerLibErrorKind_BufferOverflow)) return 0;
		node_product *= nodes[a];                             /* (at most 4096 x 2^32 - 1: no overflow) */
		if (!check(node_product <= BEAMFORMER_HIP_MAX_WARP_NODES, BeamformerLibErrorKind_BufferOverflow)) return 0;
	}
	if (!check(count * node_product <= BEAMFORMER_HIP_MAX_WARP_ENTRIES, BeamformerLibErrorKind_BufferOverflow)) return 0;
	if (!check(interpolation < BeamformerHipWarpInterpolation_Count && edge < BeamformerHipWarpEdge_Count, BeamformerLibErrorKind_InvalidAccess)) return 0;
	for (int a = 0; a < 3; a++) {
		if (!check(std::isfinite(node_first[a]), BeamformerLibErrorKind_InvalidAccess)) return 0;
		if (nodes[a] > 1 && !check(std::isfinite(node_step[a]) && node_step[a] > 0.0f, BeamformerLibErrorKind_InvalidAccess)) return 0;
	}
	for (uint64_t n = 0; n < 3 * count * node_product; n++)
		if (!check(std::isfinite(field[n]) && std::fabs(field[n]) <= BEAMFORMER_HIP_MAX_WARP_DISPLACEMENT, BeamformerLibErrorKind_InvalidAccess)) return 0;
	for (uint32_t n = 0; rotations && n < 2 * count; n++)
		if (!check(std::isfinite(rotations[n]), BeamformerLibErrorKind_InvalidAccess)) return 0;
	return warp_last_frames(count, field, nodes, node_first, node_step, rotations, interpolation, edge, image_plane_tag, first_frame_id, device_ms);
}

uint32_t beamformer_hip_copy_frame(uint32_t frame_id, void *out, uint64_t out_size)
{
	if (!check(out != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	return copy_frame(frame_id, out, out_size);
}

uint32_t beamformer_hip_get_frame_info(uint32_t frame_id, BeamformerHipFrameInfo *out)
{
	if (!check(out != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	return frame_info(frame_id, out);
}

/* host only: the criterion of every row in double, the best one (include/ogl_beamformer_hip.h: BeamformerHipFrameScore) */
uint32_t beamformer_hip_rank_frames(const BeamformerHipFrameMetrics *metrics, uint32_t count, uint32_t criterion, double *scores, uint32_t *best_index)
{
	if (!check(metrics != nullptr && best_index != nullptr && count >= 1 && criterion < (uint32_t)BeamformerHipFrameScore_Count,
	           BeamformerLibErrorKind_InvalidAccess)) return 0;
	double   best = -INFINITY;
	uint32_t best_at = 0;
	for (uint32_t i = 0; i < count; i++) {
		const BeamformerHipFrameMetrics &m = metrics[i];
		double score = -INFINITY;
		if (m.voxels != 0 && m.sum_abs2 != 0) {
			switch (criterion) {
			case BeamformerHipFrameScore_Energy:         score = m.sum_abs2; break;
			case BeamformerHipFrameScore_MeanMagnitude:  score = m.sum_abs / (double)m.voxels; break;
			case BeamformerHipFrameScore_Sharpness:      score = (double)m.voxels * m.sum_abs4 / (m.sum_abs2 * m.sum_abs2); break;
			case BeamformerHipFrameScore_GradientEnergy: score = (m.gradient2[0] + m.gradient2[1] + m.gradient2[2]) / m.sum_abs2; break;
			}
		}
		if (scores) scores[i] = score;
		if (score > best) { best = score; best_at = i; }
	}
	if (!check(best > -INFINITY, BeamformerLibErrorKind_InvalidAccess)) return 0;
	*best_index = best_at;
	return 1;
}

uint32_t beamformer_hip_display_last_frame(float threshold_db, float gamma, float db_cutoff, float *out, uint64_t out_floats)
{
	if (!out) return set_error(BeamformerLibErrorKind_InvalidAccess);
	if (!ensure_device()) return 0;
	return display_last_frame(threshold_db, gamma, db_cutoff, out, out_floats);
}

uint32_t beamformer_hip_enable_hilbert(uint32_t enable)
{
	Context &c = ctx();
	c.hilbert_enabled = enable != 0;
	for (auto &b : c.blocks) b.dirty |= Dirty_ComputePipeline;
	return 1;
}

uint32_t beamformer_hip_set_das_path(uint32_t mode) { ctx().das_path_mode = mode; return 1; }

void beamformer_hip_host_das_transform(const float min_coordinate[3], const float max_coordinate[3],
                                       int32_t points[3], float out16[16])
{
	das_transform(min_coordinate, max_coordinate, points, out16);
}

uint32_t beamformer_hip_host_hadamard(uint32_t order, float *out)
{
	std::vector<float> h = hadamard_transpose((int)order);
	if (h.empty()) return 0;
	std::memcpy(out, h.data(), sizeof(float) * h.size());
	return 1;
}

int32_t beamformer_hip_host_filter(const BeamformerFilterParameters *filter, float *taps, uint32_t capacity_floats,
                                   float *time_delay, uint32_t *complex_taps)
{
	Filter f;
	if (!filter_create(*filter, f) || f.taps.size() > capacity_floats) return -1;
	std::memcpy(taps, f.taps.data(), sizeof(float) * f.taps.size());
	if (time_delay)   *time_delay   = f.time_delay;
	if (complex_taps) *complex_taps = f.complex_taps;
	return f.length;
}

uint32_t beamformer_hip_describe_plan(uint32_t parameter_slot, BeamformerHipPlan *out)
{
	if (!valid_parameter_block(parameter_slot)) return 0;
	Plan plan;
	if (!resolved_plan(ctx().blocks[parameter_slot], plan)) return 0;
	std::memset(out, 0, sizeof(*out));
	out->stage_count = (uint32_t)plan.stages.size();
	for (size_t i = 0; i < plan.stages.size() && i < BeamformerMaxComputeShaderStages; i++) {
		const Stage &st = plan.stages[i];
		out->stages[i].kind = st.kind; out->stages[i].in_kind = st.in_kind; out->stages[i].out_kind = st.out_kind;
		for (int k = 0; k < 3; k++) { out->stages[i].in_stride[k] = st.in_stride[k]; out->stages[i].out_stride[k] = st.out_stride[k]; }
	}
	out->das_samples = plan.das_samples; out->iq_pipeline = plan.iq_pipeline;
	out->das_sampling_frequency = plan.das_sampling_frequency; out->das_time_offset = plan.das_time_offset;
	std::memcpy(out->das_voxel_transform, plan.das_voxel_transform, sizeof(out->das_voxel_transform));
	out->intermediate_bytes = plan.intermediate_bytes;
	return 1;
}

uint32_t beamformer_hip_describe_upload(uint32_t parameter_slot, uint32_t data_size, uint32_t frame_count, const void *device_pointer,
                                        BeamformerHipUploadDescription *out)
{
	if (!valid_parameter_block(parameter_slot) || !check(out != nullptr && frame_count != 0, BeamformerLibErrorKind_InvalidAccess)) return 0;
	if (frame_count > 1 && !valid_burst_count(frame_count)) return 0;
	const ParameterBlock &pb = ctx().blocks[parameter_slot];
	/* the frame against the block, as the push judges it (there is no data to look at: any non-null address passes for it) */
	if (!valid_rf_frame(pb, out, data_size)) return 0;
	Plan plan;
	if (!resolved_plan(pb, plan)) return 0;
	return describe_upload(pb, plan, data_size, frame_count, device_pointer, out) ? 1 : 0;
}

uint32_t beamformer_hip_set_hook(const char *name, const char *value)
{
	/* the two switches that are no das_select.cpp switches: how the boxes of beamformer_hip_gram_boxes_last_frames are batched, and which
	 * of its two kernels beamformer_hip_mix_field_last_frames runs (frame_ops.cpp) */
	if (name && !std::strcmp(name, "GRAM_BOXES_BUDGET")) {
		set_gram_boxes_budget(value && value[0] ? std::strtoull(value, nullptr, 0) : 0);
		return 1;
	}
	if (name && !std::strcmp(name, "BLEND_SHAPE")) {
		set_blend_shape(value && value[0] ? (std::strtoul(value, nullptr, 0) ? 1 : 0) : -1);
		return 1;
	}
	return check(set_hook(name, value), BeamformerLibErrorKind_InvalidAccess);
}

uint32_t beamformer_hip_describe_das(uint32_t parameter_slot, BeamformerHipDasDescription *out)
{
	if (!valid_parameter_block(parameter_slot) || !check(out != nullptr, BeamformerLibErrorKind_InvalidAccess)) return 0;
	Context &c = ctx();
	const ParameterBlock &pb = c.blocks[parameter_slot];
	Plan plan;
	if (!resolved_plan(pb, plan)) return 0;
	std::memset(out, 0, sizeof(*out));
	if (plan.das_index < 0) { out->path = -1; return 1; }
	uint32_t zfirst, zcount;
	shard_planes(pb, plan, zfirst, zcount);
	/* the decision for the planes that keep the first choice; where the row-end rule cuts the range (das_select.h: decide_das_parts) the
	 * planes handed to the kernel behind it are counted in row_end_planes */
	std::vector<DasDecision> parts;
	decide_das_parts(pb, plan, build_transmit_table(pb), zfirst, zcount, c.das_path_mode, parts);
	const DasDecision &d = main_part(parts);
	out->row_end_planes = row_end_planes(parts);
	out->path = d.path == DasPath_Zero ? -2 : d.path;
	std::snprintf(out->kernel, sizeof(out->kernel), "%s", das_kernel_name(d.path));
	std::snprintf(out->name, sizeof(out->name), "%s", das_path_name(d.path));
	for (int k = 0; k < DasPath_Count && k < 8; k++) std::snprintf(out->declined[k], sizeof(out->declined[k]), "%s", d.why[k].c_str());
	for (int k = 0; k < 3; k++) { out->tile_shift[k] = d.a.tile_shift[k]; out->blocks[k] = d.a.blocks[k]; }
	out->split_shift = d.a.split_shift; out->tile_walk = d.path == DasPath_Hercules ? d.herc.depth_major : (d.path == DasPath_Gather || d.path == DasPath_Staged) ? d.sep.depth_major : d.a.depth_major;
	out->tile_window_samples = d.path == DasPath_Tile ? 1u << d.a.tile_window_shift : 0u;
	if (d.path == DasPath_Gather || d.path == DasPath_Staged) {
		out->u_axis = d.sep.u_axis; out->u_shift = d.sep.u_shift; out->v_shift = d.sep.v_shift; out->window_samples = d.path == DasPath_Staged ? d.sep.window_samples : 0;
		out->uniform_tables = d.sep.uniform; out->lds_bytes = d.sep.lds_bytes; out->threads = d.sep.threads; out->channel_chunk = d.sep.channel_chunk;
	}
	out->hercules_prepared_copy = d.hercules_prepared;
	out->tile_spread_estimate = d.tile_spread;
	for (int k = 0; k < 3; k++) out->tile_estimate_shift[k] = d.tile_estimate_shift[k];
	out->row_ends = d.a.row_ends;
	out->row_end_path = -1;
	uint32_t most = 0;
	for (const DasDecision &p : parts)
		if (p.row_end_fallback && p.z_count > most) { most = p.z_count; out->row_end_path = p.path == DasPath_Zero ? -2 : p.path; }
	return 1;
}

void beamformer_hip_shutdown(void) { shutdown_device(); }

} // extern "C"
