/* das_select.h -- which DAS kernel a frame runs, and why: one ladder of rules, each a function, tried in the order decide_das lists them
 * (das_select.cpp); host only (no HIP call), shared by the executor (which launches what it says), beamformer_hip_describe_das (which
 * reports it, also without a device) and the tests (which ask instead of restating the rules).  On the single-frame decision stand the
 * routes of the multi-frame pushes (decide_burst, decide_views, decide_burst_views, decide_variants, decide_readi_image).  Also the
 * library's six diagnostic switches (beamformer_hip_set_hook). */
#ifndef BF_DAS_SELECT_H
#define BF_DAS_SELECT_H

#include "planner.h"
#include "bf_kernels.h"
#include "../../include/ogl_beamformer_hip.h"
#include <string>
#include <vector>

namespace bf {

/* BeamformerHipFrameTimings::das_path */
enum DasPath {
	DasPath_General = 0, DasPath_Gather = 1, DasPath_Staged = 2, DasPath_Factored = 3, DasPath_Hercules = 4,
	DasPath_Tile = 5,             /* das_tile.hip: the factored kernel with block-wide LDS staging */
	DasPath_Count = 6,
	DasPath_Zero = 7,             /* a family / interpolation the shader leaves at zero: the frame is cleared, no kernel */
};
const char *das_path_name(int path);      /* "LDS-staged kernel", ... */
const char *das_kernel_name(int path);    /* "das_rca_staged_kernel", ... */

/* The das path mode word (beamformer_hip_set_das_path): a kernel request in the low nibble (BeamformerHipDasPath_Automatic ..
 * _HerculesAnyWidth), flags above it (BeamformerHipDasPath_NoChannelSplit ...). */
constexpr uint32_t kDasPathRequestMask = 0xF;
inline uint32_t das_path_request(uint32_t mode) { return mode & kDasPathRequestMask; }

constexpr uint32_t kStagedMinTransmits = 6;      /* das_staged.hip by default from this many transmits per channel (tools/staged_threshold.py,
                                                    profiles/r03_staged_threshold.json: 1.29 of the gather kernel's time at 4 transmits, 1.01 at 6,
                                                    1.0 at 8, 0.88 at 12, 0.75 at 16, 0.69-0.71 at 32-75; round 2's pass: 1.15, -, 0.91, 0.84, 0.75) */

constexpr uint32_t kBurstMinFrames = 5;          /* das_burst.hip takes bursts of this many frames and more.  Wall time per frame of one burst on the
                                                    burst kernel over N single pushes, upload included (tools/burst_rate.py, profiles/burst_rate.json),
                                                    by N -- config 1 (64 ch, 1 tx, 256 x 256): 2: 1.16, 4: 0.88, 8: 0.71, 16: 0.53, 64: 0.51, 256: 0.33;
                                                    the same plane with 2 transmits: 2: 1.37, 4: 1.02, 8: 0.78, 16: 0.60, 64: 0.75, 256: 0.54.  Two
                                                    frames are one group of four slots, half of them aliased, on a quarter of the waves the single
                                                    kernel's channel split launches: slower; four are level; from five on the burst is taken (the
                                                    per-frame DAS route under the same batching: 1.04 / 1.24 at 2, 1.00 / 1.08 at 4, 0.95 / 1.00 at 8) */

constexpr uint32_t kReadiSweepMinFrames = 5;     /* das_readi_burst_kernel (das_burst.hip) takes READI sweeps of this many frames and more: the smallest
                                                    measured frame count from which the sweep on the kernel is not slower than the sweep on the
                                                    per-frame route by more than three times that route's run-to-run spread (tools/readi_rate.py,
                                                    profiles/readi_rate.json).  Wall time per frame of the kernel over the per-frame route, upload
                                                    included, by N -- G = 4: 5: 0.66, 6: 0.58, 8: 0.46, 16: 0.37, 64: 0.34; G = 8: 5: 0.69, 8: 0.49,
                                                    16: 0.35, 64: 0.37; G = 16: 5: 0.68, 16: 0.36, 64: 0.35; over N x (parameter push + single push):
                                                    0.55-0.60 at 5, 0.28-0.32 at 64.  Fewer than 5 frames were not measured on the kernel (the value
                                                    in force, the burst kernel's, sent them down the per-frame route) */

/* Diagnostic switches (none is needed in production, all default off): set through beamformer_hip_set_hook ONLY -- the library
 * reads no environment variable.  They select among code paths that ship anyway (the range-checked loop every boundary wave takes,
 * the LDS-table form every non-64 x 16 tile takes, ...) so that the tests can aim at each of them.  `version` counts changes:
 * cached decisions carry it. */
struct Hooks {
	uint64_t    version = 1;
	int         staged_shape[3] = {0, 0, 0};   /* STAGED_SHAPE="u,v,w": only 2^u x 2^v tiles with 2^w-sample windows */
	bool        staged_shape_set = false;
	bool        staged_checked = false;        /* STAGED_CHECKED: the range-checked loop for every wave (it also counts window violations) */
	bool        staged_nouniform = false;      /* STAGED_NOUNIFORM: transmit tables in LDS also where the wave-uniform form applies */
	uint64_t    staged_table_cap = 2ull << 30; /* STAGED_TABLE_CAP=bytes: largest global transmit table taken (0 forces the fallback) */
	bool        debug = false;                 /* DEBUG: one line per staged plan on stderr */
	bool        scratch_poison = false;        /* SCRATCH_POISON: both intermediate buffers and the frame's ring slot filled with 0xFF bytes (a NaN
	                                              in binary16 and in f32) at the start of every frame, so that whatever a stage reads without
	                                              this frame having written it turns into NaN (executor.cpp) */
};
Hooks &hooks();
bool   set_hook(const char *name, const char *value);       /* value null or "" = unset; false: unknown name */
const char *const *hook_names();                             /* null-terminated */

struct DasDecision {
	bool     valid = false;
	uint64_t generation = 0, hooks_version = 0;              /* what it was computed for */
	uint32_t z_first = 0, z_count = 0, mode = 0;
	uint32_t mode_asked = 0;             /* decide_das_parts: the caller's mode (a fallback part is decided under another) */
	BfDasArgs a{};                      /* everything but the device pointers */
	float     tile_spread = 0.f;         /* das_tile.hip: the estimated spread of a tile of 2^tile_estimate_shift voxels (0: not a factored-kernel frame) */
	uint32_t  tile_estimate_shift[3] = {0, 0, 0};
	BfDasArgs general{};                /* the same with the general kernel's tile geometry (no channel split): what the pair count runs with */
	int      path = DasPath_General;
	int      depth_axis = 2;
	BfSeparableArgs sep{};              /* Gather: its geometry; Staged: the staged kernel's */
	BfSeparableArgs sep_gather{};       /* Staged: what the gather kernel would run with -- the fallback when the staged kernel cannot be launched */
	bool            has_lds_tables = false;
	BfSeparableArgs sep_lds_tables{};   /* Staged with wave-uniform (global) tables: the shape with the tables in LDS, used when the table cannot be allocated */
	BfHerculesArgs  herc{};
	bool     hercules_prepared = false; /* Hercules: read the {sample, difference} / polynomial copy of the DAS input */
	uint64_t das_input_bytes = 0;
	std::string why[DasPath_Count];     /* why each kernel was not taken ("" for the one that runs and for kernels not considered) */
	bool     row_end_fallback = false;  /* decide_das_parts: these planes went to the kernel BEHIND the staged one because a term can reach an end of its RF row */
};

/* per-transmit constants of das.glsl:172-202 (host side; the executor uploads them) */
std::vector<BfTransmit> build_transmit_table(const ParameterBlock &pb);

/* Fills `out` for one DAS launch over planes [z_first, z_first + z_count) of the block's grid under das path `mode`
 * (beamformer_hip_set_das_path).  Pure host arithmetic. */
void decide_das(const ParameterBlock &pb, const Plan &plan, const std::vector<BfTransmit> &transmits,
                uint32_t z_first, uint32_t z_count, uint32_t mode, DasDecision &out);

/* The same, cut along z where the ROW-END rule (das_exact.h) asks for it.  The LDS-staged kernels (das_staged*.hip) and the block-staged
 * factored kernel (das_tile.hip) decide sample_rf's range test by their own index and carry no exact evaluation of the terms at the ends
 * of an RF row (their checked loops run at their register limit; every other kernel evaluates those terms itself).  They therefore get only planes on which provably no in-aperture term
 * comes within reach of an end of its row -- a host bound per plane, in double precision, over the plane's corners; on every real
 * acquisition whose rows do not end inside the image that is all of them, and `parts` holds ONE decision.  Otherwise the range is cut into
 * runs of planes: clear runs keep their kernel, the others go to the kernel behind it (gather / factored / general, which evaluate
 * row-end terms exactly).  Parts are contiguous, in z order, and cover [z_first, z_first + z_count). */
void decide_das_parts(const ParameterBlock &pb, const Plan &plan, const std::vector<BfTransmit> &transmits,
                      uint32_t z_first, uint32_t z_count, uint32_t mode, std::vector<DasDecision> &parts);
/* How a burst of frame_count frames runs (beamformer_hip_describe_burst): das_burst.hip in one launch when the single-frame decision
 * `parts` is ONE part on the general kernel, the family is RCA, frame_count >= kBurstMinFrames and mode does not carry
 * BeamformerHipDasPath_NoBurstKernel; else the single-frame launch(es) once per frame.  `a`: the burst kernel's arguments (the general
 * kernel's tiles without the channel split). */
struct BurstDecision {
	bool        burst_kernel = false;
	bool        readi_sweep = false;         /* the push is a READI sweep: burst_kernel names das_readi_burst_kernel */
	int         single_path = DasPath_General;
	uint32_t    frames_per_thread = 1, das_launches = 0, stage_launches = 0;
	uint32_t    min_frames = kBurstMinFrames;   /* the threshold that was applied */
	std::string reason;
	BfDasArgs   a{};
};
/* readi_sweep: the push is a READI sweep (beamformer_hip_describe_readi_sweep) -- frame k under its own readi_group.  Its kernel,
 * das_readi_burst_kernel, takes it when `parts` is ONE part on the general kernel, the family is READI, frame_count >=
 * kReadiSweepMinFrames and mode does not carry BeamformerHipDasPath_NoBurstKernel; else the single-frame launch(es) once per frame,
 * each with its frame's group.  A plain burst (readi_sweep false) of a READI block never takes a kernel of das_burst.hip. */
void decide_burst(const ParameterBlock &pb, const Plan &plan, const std::vector<BfTransmit> &transmits, const std::vector<DasDecision> &parts,
                  uint32_t z_first, uint32_t z_count, uint32_t mode, uint32_t frame_count, BurstDecision &out, bool readi_sweep = false);

/* das_views.hip takes the eligible views of a push when their 256-voxel tiles number at least this.  PROVISIONAL: the smallest tile
 * count at which the views kernel is not slower than the per-view route by more than three times that route's run-to-run spread, to be
 * read off profiles/views_rate.json (tools/views_rate.py) -- see the note beside that file in profiles/README.md. */
constexpr uint32_t kViewsMinTiles = 2;

/* One grid of a views push: BeamformerHipView without its tag. */
struct ViewGrid {
	float    transform[16];            /* as BeamformerParameters::das_voxel_transform */
	uint32_t points[3];                /* each >= 1 */
};
/* The block's plan on a view's grid: `plan` with the view's points and voxel transform (FORCES / UFORCES: pre-multiplied by the transducer
 * transform as build_plan does, beamformer_core.c:913-915).  What decide_das_parts takes for that view. */
void plan_on_view(const ParameterBlock &pb, const ViewGrid &view, Plan &plan);

/* How a views push runs (beamformer_hip_describe_views): every view gets its own decide_das_parts -- its single-frame decision, parts[v].
 * A view is ELIGIBLE for das_views.hip when that decision is one part on the general kernel, the family is RCA and mode does not carry
 * BeamformerHipDasPath_NoViewsKernel; the eligible views run in ONE launch when their 256-voxel tiles (no channel split) number at least
 * kViewsMinTiles, or mode carries BeamformerHipDasPath_PreferViewsKernel.  Every other view runs its single-frame launch(es). */
struct ViewsDecision {
	std::vector<std::vector<DasDecision>> parts;      /* per view */
	std::vector<uint8_t>   taken;                     /* per view: 1 = in the views kernel's launch */
	std::vector<BfViewRow> rows;                      /* the taken views, in view order (out_offset: filled by the executor) */
	std::vector<uint32_t>  first_block;               /* rows.size() + 1 */
	uint32_t    kernel_views = 0, kernel_tiles = 0, das_launches = 0;
	BfDasArgs   a{};                                  /* the views kernel's arguments: the general kernel's without grid and channel split */
	std::string reason;
};
void decide_views(const ParameterBlock &pb, const Plan &plan, const std::vector<BfTransmit> &transmits, const ViewGrid *views, uint32_t view_count,
                  uint32_t mode, ViewsDecision &out);

/* das_burst_views_kernel (das_burst_views.hip) takes burst views pushes of this many RF frames and more: the smallest measured frame
 * count from which the push on the fused kernel is not slower than the views kernel per RF frame (flag 0x400) by more than three times
 * that route's run-to-run spread (tools/burst_views_rate.py, profiles/burst_views_rate.json: min_frames_from_this_table).  Wall time
 * per queued frame of the fused kernel over that route, upload included, by N -- 2 planes of 256 x 1 x 256: 5: 0.57, 8: 0.49, 16: 0.37,
 * 64: 0.44, 256: 0.31; 3 planes: 5: 0.69, 8: 0.51, 64: 0.40, 256: 0.31; 16 patches of 16 x 1 x 16: 5: 0.52, 16: 0.36, 256: 0.21; over
 * K x (parameter push + burst push): 0.35-0.75 on the planes, 0.06-0.10 on the patches.  Fewer than 5 frames were not measured on the
 * kernel (the value in force, the burst kernel's break-even, sent them down the per-frame route). */
constexpr uint32_t kBurstViewsMinFrames = 5;

/* How a burst views push of frame_count RF frames on view_count grids runs (beamformer_hip_describe_burst_views): a ladder.
 *   rung 1  the fused kernel: the views das_views.hip is eligible for (decide_views: one part on the general kernel, RCA family), ALL in
 *           one launch whatever their tile count, when frame_count >= kBurstViewsMinFrames and mode carries neither
 *           BeamformerHipDasPath_NoBurstKernel (0x400) nor _NoViewsKernel (0x800); every other view its single-frame launch(es) per RF frame;
 *   rung 2  below the threshold or under 0x400, 0x800 absent: per RF frame the views push's own DAS step under decide_views' unchanged rules;
 *   rung 3  under 0x800, or where no view is eligible: every (view, RF frame) its view's single-frame launch(es).
 * `views`: the per-view decisions, and for rungs 1 and 2 the taken views' rows and prefix table. */
struct BurstViewsDecision {
	ViewsDecision views;
	uint32_t    rung = 3, kernel_views = 0, frame_kernel_views = 0, frames_per_thread = 1, das_launches = 0, stage_launches = 0;
	uint32_t    min_frames = kBurstViewsMinFrames;
	std::string reason;
};
void decide_burst_views(const ParameterBlock &pb, const Plan &plan, const std::vector<BfTransmit> &transmits, const ViewGrid *views, uint32_t view_count,
                        uint32_t mode, uint32_t frame_count, BurstViewsDecision &out);

/* das_variants.hip takes the eligible variants of a push when they number at least kVariantsMinVariants, or when variants x 256-voxel
 * tiles of the block's grid number at least kVariantsMinTiles: each the smallest measured count from which the push on the kernel is not
 * slower than the push on the per-variant route by more than three times that route's run-to-run spread, in every row at that count and
 * above (tools/variants_rate.py, profiles/variants_rate.json: min_variants_from_this_table, min_tiles_from_this_table; the tool's runs on
 * the MI355X gave 4 and 8 variants, 512 and 1024 tiles -- four variants on a patch, two on the plane are within a few us either way --
 * and the larger figures are in force, with which the rule holds in every run).  The break-even was expected to follow variants x tiles
 * alone, from about 2; measured, it follows the NUMBER OF VARIANTS: the fused launch's DAS segment has a floor of about 36 us whatever it
 * computes (its table transfer, and one thread per voxel walking all channels where the single-frame general kernel splits them over up
 * to 16 waves), a single-frame launch costs 9 - 14 us and each further one 6 - 11 us more.  DESIGN 3.1f has the table. */
constexpr uint32_t kVariantsMinVariants = 8;
constexpr uint32_t kVariantsMinTiles = 1024;

/* One candidate of a variants push: BeamformerHipDasVariant. */
struct DasVariant {
	float speed_of_sound, time_offset, f_number;   /* as the BeamformerParameters fields of those names (time_offset: the block field, not the plan's sum) */
};
/* The block with the three fields replaced, and its plan: `plan` -- the block's own resolved plan -- with das_time_offset resolved anew,
 * in the planner's own order of additions (planner.cpp: the block field, then every pre-DAS filter's delay in stage order), so that it is
 * the float a block carrying that value plans to.  The three values reach nothing else of a plan, and of a frame only the DAS decision
 * (decide_das: inv_speed_of_sound, speed_of_sound, time_offset, f_number, edge_margin, and the kernel choices and tables that follow from
 * them).  The derived plan leaves out the Hadamard matrices, which no DAS decision reads. */
void derive_variant(const ParameterBlock &pb, const Plan &plan, const DasVariant &variant, ParameterBlock &derived_pb, Plan &derived_plan);

/* How a variants push runs (beamformer_hip_describe_variants): every variant gets decide_das_parts of its derived block -- its
 * single-frame decision, parts[v] (known[v] given: that decision from an earlier call for the same block, plan, variant, mode and hooks,
 * taken as it is).  A variant is ELIGIBLE for das_variants.hip when that decision is one part on the general kernel, the family is RCA
 * and mode does not carry BeamformerHipDasPath_NoVariantsKernel; the eligible variants run in ONE launch when they, times the 256-voxel
 * tiles of the grid (no channel split), number at least kVariantsMinTiles, when they number at least kVariantsMinVariants, or when mode
 * carries BeamformerHipDasPath_PreferVariantsKernel.
 * Every other variant runs its single-frame launch(es) on the shared DAS input. */
struct VariantsDecision {
	std::vector<std::vector<DasDecision>> parts;      /* per variant */
	std::vector<uint8_t>      taken;                  /* per variant: 1 = in the variants kernel's launch */
	std::vector<BfVariantRow> rows;                   /* the taken variants, in variant order (out_offset: filled by the executor) */
	uint32_t    kernel_variants = 0, kernel_tiles = 0, das_launches = 0;      /* kernel_tiles: blocks of the fused launch */
	BfDasArgs   a{};                                  /* the variants kernel's arguments: the general kernel's on 256-voxel tiles, no channel split;
	                                                     row_ends the OR over the taken variants */
	std::string reason;
};
void decide_variants(const ParameterBlock &pb, const Plan &plan, const std::vector<BfTransmit> &transmits, const DasVariant *variants, uint32_t variant_count,
                     uint32_t mode, VariantsDecision &out, const std::vector<DasDecision> *const *known = nullptr);

/* READI image (beamformer_hip_push_data_readi_image_with_compute).  READI_FORCES is FORCES with transmit element
 * tx_group * acquisition_count + tx_event and every term signed by Hadamard[readi_group * G + tx_group] (das.glsl:288-366), and everything
 * behind the sign is linear in the samples: the sum of a sequence's partial frames is ONE frame of the DERIVED block -- the same block with
 * acquisition_kind FORCES, acquisition_count G x A, READI off, not sparse (the shader's READI branch ignores sparse_elements) -- on the
 * DAS input decoded across the acquisitions (readi_decode.hip).  derive_readi_image gives that block and its plan: the block's own
 * resolved plan -- das_samples, sampling frequency, time offset, IQ pipeline, grid, voxel transform and stages as they are -- changed only
 * in the acquisition count and the family.  `pb` is a READI block with G x A <= BeamformerMaxEmissionsCount (lib_api.cpp has checked). */
void derive_readi_image(const ParameterBlock &pb, const Plan &plan, ParameterBlock &derived_pb, Plan &derived_plan);
/* How an image push of frame_count RF frames runs, `parts` being decide_das_parts of the derived block: the decode in one launch, then
 * the derived block's single-frame launch(es), once. */
struct ReadiImageDecision {
	uint32_t    transmit_count = 0, das_launches = 0, stage_launches = 0, decode_launches = 0;
	int         path = -1;            /* the derived block's main part (DasPath); -1: no DAS stage */
	std::string reason;
};
void decide_readi_image(const Plan &derived_plan, const std::vector<DasDecision> &parts, uint32_t group_count, uint32_t frame_count, ReadiImageDecision &out);

/* planes of `parts` that took the fallback */
uint32_t row_end_planes(const std::vector<DasDecision> &parts);
/* the part with the most planes (what a frame "ran on" in one word) */
const DasDecision &main_part(const std::vector<DasDecision> &parts);

} // namespace bf
#endif
