/* bf_kernels.h -- launch interface between the host executor (C++) and the gfx950 kernels.
 * Plain structs passed by value as kernel arguments: they replace the reference's Vulkan
 * specialization constants ("Bake" structs, generated/beamformer.c:176-249) and push
 * constants (generated/beamformer.c:251-279). */
#ifndef BF_KERNELS_H
#define BF_KERNELS_H

#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime_api.h>

/* generated/beamformer.c:489-521 */
static const int bf_kind_byte_size[6]     = {2, 4, 4, 8, 2, 4};
static const int bf_kind_element_size[6]  = {2, 2, 4, 4, 2, 2};
static const int bf_kind_element_count[6] = {1, 2, 1, 2, 1, 2};
static const int bf_kind_complex[6]       = {0, 1, 0, 1, 0, 1};
enum { BF_BASE_I16 = 0, BF_BASE_F32 = 1, BF_BASE_F16 = 2 };
static const int bf_kind_base[6] = {BF_BASE_I16, BF_BASE_I16, BF_BASE_F32, BF_BASE_F32, BF_BASE_F16, BF_BASE_F16};

/* per-transmit constants prepared on the host from focal_vectors / orientations
 * (das.glsl:172-202): 32 bytes each, read through wave-uniform (scalar) loads */
typedef struct {
	float    sin_a, cos_a;       /* of the steering angle */
	float    focus_x, focus_z;   /* focal_depth * (sin, cos); unused for plane waves */
	uint32_t flags;              /* BF_TX_* */
	float    pad[3];
} BfTransmit;
enum {
	BF_TX_ROWS    = 1u << 0,   /* transmit orientation == Rows (project on y,z) */
	BF_RX_ROWS    = 1u << 1,   /* receive  orientation == Rows */
	BF_TX_NONE    = 1u << 2,   /* transmit orientation == None: distance 0 */
	BF_TX_PLANE   = 1u << 3,   /* focal depth is +-inf */
	BF_RX_COLUMNS = 1u << 4,   /* receive orientation == Columns (HERCULES test, das.glsl:238) */
};

enum { BF_DAS_RCA = 0, BF_DAS_HERCULES = 1, BF_DAS_FORCES = 2, BF_DAS_READI = 3 };

typedef struct {
	float xdc_transform[16];
	float voxel_transform[16];
	float pitch[2];
	const void       *rf;             /* [channel][transmit][sample], float or float2 */
	void             *out;            /* float or float2 per voxel of the shard */
	const BfTransmit *transmits;      /* [acquisition_count] */
	const int16_t    *sparse_elements;
	const uint16_t   *readi_hadamard; /* binary16 bits, G*G */
	unsigned long long *pair_counter; /* COUNT kernels only */
	uint32_t *tile_counters;          /* das_tile.hip: [0] += (block, channel chunk) pairs that ran out of staged windows, [1] += those that took the gather loop; or null */
	int32_t  family, interpolation, complex_data, coherency_weighting;
	int32_t  acquisition_count, channel_count, sample_count, sparse;
	float    sampling_frequency, inv_sampling_frequency, demodulation_frequency;
	float    inv_speed_of_sound, time_offset, f_number;
	float    speed_of_sound;          /* with inv_speed_of_sound: div_speed_of_sound() of das_common.h */
	float    turns_per_sample;        /* demodulation_frequency / sampling_frequency: IQ phase per sample, in turns */
	float    first_transmit_weight;   /* HERCULES: 1/sqrt(acquisition_count) (das.glsl:272-273) */
	uint32_t size[3];                 /* whole output grid */
	uint32_t z_first, z_count;        /* shard of the grid computed by this launch */
	uint32_t readi_group_count, readi_group;
	uint32_t tile_shift[3];           /* log2 of the block's voxel tile extent per axis (256 voxels, or 64 with a channel split) */
	uint32_t split_shift;             /* log2 K: K waves of a block share 64 voxels, each summing C/K channels */
	uint32_t blocks[3];               /* blocks per axis */
	uint32_t depth_major;             /* tile walk: 1 = z fastest (consecutive tiles share a lateral column), 2 = y fastest (view planes:
	                                     depth lies along voxel y), 3 = view planes in XCD-balanced bands (bf_plane_walk), 0 = x, y, z */
	uint32_t band_rows;               /* depth_major == 3: tile rows per band */
	uint32_t zero_offset;             /* factored kernel: byte offset (from rf) of >= 32 zero bytes the host keeps
	                                     behind the DAS input, the gather target of out-of-range lanes */
	uint32_t tile_window_shift;       /* das_tile.hip: log2 of the staged window length (5 or 6) */
	float    edge_margin;             /* samples: a term whose index comes this close to an end of sample_rf's valid range is decided by the
	                                     shader's own expression, evaluated exactly (das_exact.h); 2^-19 of the largest index magnitude */
	uint32_t row_ends;                /* 1: some in-aperture term of this launch may come within reach of an end of its RF row (a host bound over the
	                                     launch's planes, das_select.cpp; 1 also where no bound is implemented).  The factored and HERCULES kernels
	                                     have an instantiation without any row-end code for launches where it is 0 */
} BfDasArgs;

/* ensemble form of the general kernel (das_burst.hip): frames a thread carries through one walk of its (channel, transmit) terms */
#define BF_BURST_FRAMES_PER_THREAD 4u
typedef struct {
	uint32_t frame_count;             /* frames of the launch: frame f reads BfDasArgs.rf + f * rf_stride and writes BfDasArgs.out + f * out_stride */
	uint32_t pad;
	uint64_t rf_stride, out_stride;   /* bytes */
} BfBurstArgs;
/* READI sweep form (das_burst.hip: das_readi_burst_kernel): a burst whose frame f is beamformed with row groups[f] of the Hadamard
 * matrix (BfDasArgs.readi_group is not read).  The ids are validated on the host (all below readi_group_count); the kernel trusts them. */
typedef struct {
	BfBurstArgs     burst;
	const uint32_t *groups;           /* [burst.frame_count], device */
} BfReadiSweepArgs;

/* READI image (readi_decode.hip: readi_image_decode_kernel): the DAS inputs of `frames` group acquisitions, frame k in_frame_bytes behind
 * frame k - 1, each [channel][slab_floats] float32 (a slab: [acquisition][sample], complex samples as pairs of floats), decoded into
 * out[channel][t][slab_floats], t < group_count: out[c][t] = sum over k, in that order, of H[groups[k]][t] * in_k[c].  The ids are
 * validated on the host (all below group_count); the kernel trusts them. */
typedef struct {
	const void     *in;
	void           *out;
	const uint32_t *groups;           /* [frames], device */
	const uint32_t *hadamard;         /* group_count^2 entries of +-1 as binary16 (row g entry t at g * group_count + t), read two to a word */
	uint64_t        in_frame_bytes, slab_floats;
	uint32_t        frames, group_count, channels, pad;
} BfReadiDecodeArgs;

/* views form of the general kernel (das_views.hip): one DAS input beamformed on several grids by one launch.  A row holds what differs
 * from view to view; everything else is the launch's BfDasArgs.  128 bytes, read through wave-uniform (scalar) loads. */
typedef struct {
	float    voxel_transform[16];
	uint32_t size[3];                 /* the view's grid (z_first = 0, z_count = size[2]) */
	uint32_t tile_shift[3];           /* 256-voxel tiles, no channel split */
	uint32_t blocks[3];
	uint32_t depth_major;             /* 0, 1 or 2: the view's own walk order (a view plane's balanced bands, 3, become 2: no XCD dealing here) */
	uint32_t band_rows;
	uint32_t pad0;
	uint64_t out_offset;              /* bytes from BfDasArgs.out to the view's frame */
	uint64_t out_stride;              /* das_burst_views_kernel: bytes from a view's frame of one RF frame to its frame of the next (das_views_kernel
	                                     does not read it) */
} BfViewRow;
#ifdef __cplusplus
static_assert(sizeof(BfViewRow) == 128 && offsetof(BfViewRow, size) == 64 && offsetof(BfViewRow, out_offset) == 112 && offsetof(BfViewRow, out_offset) % 8 == 0 &&
              offsetof(BfViewRow, out_stride) == 120,
              "BfViewRow: 128 bytes, the same on the host that fills it and in the kernel that reads it");
#endif
typedef struct {
	const BfViewRow *rows;            /* [view_count], device */
	const uint32_t  *first_block;     /* [view_count + 1], device: view v owns block ids first_block[v] .. first_block[v + 1] - 1 */
	uint32_t view_count, pad;
} BfViewsArgs;

/* variants form of the general kernel (das_variants.hip): one DAS input beamformed on the launch's own grid under several sets of DAS
 * scalars.  A row holds what differs from variant to variant -- the five fields of BfDasArgs that speed_of_sound, time_offset and
 * f_number reach, as the host fills them for a block carrying those values (das_select.cpp: decide_das), and the variant's frame;
 * everything else is the launch's BfDasArgs.  32 bytes, read through wave-uniform (scalar) loads. */
typedef struct {
	float    speed_of_sound, inv_speed_of_sound;
	float    time_offset;             /* resolved: the block field plus the filters' delays */
	float    f_number;
	float    edge_margin;
	uint32_t pad0;
	uint64_t out_offset;              /* bytes from BfDasArgs.out to the variant's frame */
} BfVariantRow;
#ifdef __cplusplus
static_assert(sizeof(BfVariantRow) == 32 && offsetof(BfVariantRow, out_offset) == 24,
              "BfVariantRow: 32 bytes, the same on the host that fills it and in the kernel that reads it");
#endif

/* channel-paired staged kernel (uniform = 2): the LDS holds the 64-element blocks (two channels' 32-sample windows) of at most this
 * many transmits at a time -- a multiple of 4 whose block indices, plus the two elements in front, stay below 4096 (the tap address
 * is a 16-bit shift of the element index) */
#define BF_STAGED_PAIRED_GROUP_MAX 60u
/* ... and the block's LDS must leave room for a second block on the CU (160 KB) */
#define BF_STAGED_PAIRED_LDS_BUDGET (80u * 1024u)

#ifdef __HIPCC__
#define BF_HOST_DEVICE __host__ __device__
#else
#define BF_HOST_DEVICE
#endif
/* dynamic LDS of the channel-paired form: the windows of the largest group (+ two elements in front, a zero element behind), the
 * receive table of a chunk of channels (an odd chunk gets a zero partner), the transmits' floors, the channels' floors and row offsets */
static inline BF_HOST_DEVICE uint32_t bf_staged_paired_lds_bytes(uint32_t group, uint32_t channel_chunk, uint32_t a4)
{
	const uint32_t lds = 16u * (group * 64u + 3u) + 16u * (((channel_chunk + 1u) & ~1u) << 5) + 4u * (a4 + 2u * (channel_chunk + 2u)) + 128u;
	return (lds + 15u) & ~15u;
}
/* staging passes of a group: 1024 threads copy 1024 window elements = 16 transmits' blocks per pass (a group of one pass runs as two:
 * the one-pass instance of the kernel spills) */
static inline BF_HOST_DEVICE uint32_t bf_staged_paired_passes(uint32_t group)
{
	const uint32_t passes = (group + 15u) / 16u;
	return passes < 2u ? 2u : passes;
}
/* THE split of a4 padded transmits (a multiple of 4) into the groups the channel-paired form stages one after the other -- the plan
 * (das_select.cpp), the launcher and the kernel (das_staged.hip) all ask here.  At most two groups, g0 >= g1 (g1 = 0: one group), both
 * multiples of 4, neither above BF_STAGED_PAIRED_GROUP_MAX nor above what the LDS budget leaves beside the receive table of
 * `channel_chunk` channels.  Of the splits that fit, the one with the fewest staging passes (every wave of the block waits at the round's
 * barrier for the slowest pass, kept or not: 76 transmits are 48 + 28 = 3 + 2 passes where halves of 40 + 36 are 3 + 3); among those a
 * first group of whole passes, then the smaller first group (less LDS).  The transmits of group 0 are 0 .. g0 - 1, group 1 the rest: they
 * are accumulated in index order whatever the split, so it changes no bit of a frame.  False: no such split (the form is not taken). */
static inline BF_HOST_DEVICE bool bf_staged_paired_split(uint32_t a4, uint32_t channel_chunk, uint32_t *g0, uint32_t *g1)
{
	uint32_t gmax = BF_STAGED_PAIRED_GROUP_MAX;
	while (gmax >= 4u && bf_staged_paired_lds_bytes(gmax, channel_chunk, a4) > BF_STAGED_PAIRED_LDS_BUDGET) gmax -= 4u;
	*g0 = *g1 = 0u;
	if (a4 < 4u || (a4 & 3u) || gmax < 4u || a4 > 2u * gmax) return false;
	if (a4 <= gmax) { *g0 = a4; return true; }
	uint32_t best_key = ~0u;
	for (uint32_t first = gmax; 2u * first >= a4; first -= 4u) {
		const uint32_t key = (bf_staged_paired_passes(first) + bf_staged_paired_passes(a4 - first)) * 256u + ((first & 15u) ? 128u : 0u) + first;
		if (key < best_key) { best_key = key; *g0 = first; *g1 = a4 - first; }
	}
	return true;
}

/* tile geometry of the separable-delay fast path (das_separable.hip) */
typedef struct {
	uint32_t u_axis;          /* output axis (0 = x, 1 = y) the receive aperture runs along */
	uint32_t u_shift, v_shift;/* log2 of the tile extent along the receive / transmit axis */
	uint32_t threads;         /* (1 << u_shift) * (1 << v_shift): 256, 512 or 1024 */
	uint32_t channel_chunk;   /* channels per receive-table rebuild */
	uint32_t lds_bytes;       /* 16 * (channel_chunk << u_shift) + 16 * (transmits << v_shift) */
	uint32_t tiles[3];        /* tiles along u, along v, z planes of the shard */
	uint32_t depth_major;     /* tile walk: 1 = z fastest (consecutive tiles share a lateral column), 0 = x, y, z */
	uint32_t walk_columns;    /* depth_major: columns adjacent along u that are walked together (bf_column_walk): 4, 2 or 1, a divisor of tiles[0] */
	uint32_t window_shift;    /* staged kernel: log2 of the RF window (samples) copied to LDS per transmit */
	uint32_t zero_offset;     /* byte offset (from BfDasArgs.rf) of >= 32 zero bytes the host keeps behind
	                             the DAS input: where out-of-range lanes gather from */
	/* staged kernel (complex, linear), 64 x 16 tiles with x along the receive axis: the transmit delays and phasors of a wave are
	 * uniform and come from a global table (bf_launch_das_staged_tables writes it per frame) through scalar loads.
	 * 32 x 32 tiles, 32-sample windows (uniform = 2, the channel-paired form): a lane beamforms rows w and w + 16 of the tile for
	 * one channel of a pair, so a wave again shares its transmit rows (two of them) and reads them from a global table */
	uint32_t uniform;         /* 1: use `tables` (64 x 16 tiles); 2: the channel-paired form, `tables` in its row-pair layout */
	uint32_t window_samples;  /* 32 or 64 (= 1 << window_shift) */
	uint32_t table_stride;    /* bytes per (lateral tile row, plane) slice: 4 A4 + 16 + 16 (A4 / 4) 48 (uniform = 1) or
	                             4 A4 + 16 + 16 (A4 / 2) 48 (uniform = 2), A4 = transmits rounded up to 4 */
	void    *tables;          /* tiles[1] * tiles[2] slices */
	uint32_t *violations;     /* staged kernels, range-checked loop: incremented once per wave and channel in which some term's window
	                             position fell outside the staged window -- a violated host bound (plan_staged) made loud; may be null */
} BfSeparableArgs;

/* geometry of the HERCULES fast path (das_hercules.hip): lanes of a wave lie along the output's x
 * axis; the array axis that moves with x is the OUTER loop, the other one (a function of the
 * output row y alone) the INNER loop, served from a wave-uniform table */
typedef struct {
	float   *table;           /* [size[1]][table_pitch]: squared lateral distance row y <-> inner element n */
	float   *extremes;        /* [size[1]][2]: min and max of each table row */
	uint32_t table_pitch;     /* floats per row, >= inner_count + 8 (the kernel prefetches a batch ahead) */
	uint32_t inner_count, outer_count;
	uint32_t inner_coord;     /* transducer coordinate of the inner axis: 0 = x, 1 = y */
	uint32_t inner_is_transmit;   /* inner loop walks decoded transmit elements (else receive channels) */
	uint32_t tiles[3];        /* 64-voxel x segments, groups of `rows` output rows, z planes of the shard */
	uint32_t rows;            /* output rows (= waves) of a block: 4, 8 or 16; they walk the outer elements in step (a barrier per element) */
	uint32_t depth_major;     /* tile walk: 1 = z fastest, 2 = y fastest (view planes), 3 = balanced bands (bf_plane_walk), 0 = x, y, z */
	uint32_t band_rows;       /* depth_major == 3: tile rows per band */
	uint32_t zero_offset;     /* byte offset (from BfDasArgs.rf) of >= 32 zero bytes behind the DAS input */
	/* The kernel measures squared distances in units of unit_scale2 (a float within 1e-3 of 1) and converts a
	 * distance to samples with samples_per_unit: the host picks the pair so that samples_per_unit x
	 * sqrt(unit_scale2) equals fs / c to ~1e-11 (plan_hercules), because the rounding of a single fs/c constant
	 * would be a relative bias common to every tap -- 2e-8, i.e. up to 1e-4 rad of demodulation phase on a
	 * coherent peak -- and a per-pair division costs 9 % of the kernel. */
	float    unit_scale2, samples_per_unit;
	void    *pairs;           /* IQ + linear interpolation: scratch for the {sample, difference to the next} copy of the DAS input (16 bytes per
	                             sample + 32 zero bytes), or null: the kernel then reads BfDasArgs.rf as every other kernel does */
	uint32_t phase_local;     /* IQ: the indices of one inner loop stay within ~400 turns of demodulation phase of each other, so the
	                             kernel subtracts one integer per lane and outer element instead of taking v_fract per pair */
} BfHerculesArgs;

typedef struct {
	const void *raw; void *out;
	const int16_t *channel_mapping;   /* device, [channels] */
	uint64_t in_row_bytes, out_row_bytes;
	uint32_t channels;
	int32_t  a1s2, base;              /* A1S2 contrast reduction on BF_BASE_* scalars */
	uint32_t a1s2_scalars;            /* sample_count * element_count */
	uint32_t frames;                  /* a burst (executor.cpp push_burst): frames of the launch, 0 or 1 = one; frame f reads and writes f * the strides below further on */
	uint64_t in_frame_bytes, out_frame_bytes;
} BfIngestArgs;

/* Bytes a lane of ingest_copy_kernel moves per step: the widest of 16, 4 and 2 that divides both row strides, both frame strides and
 * both addresses.  stages.hip launches by it and executor.cpp's decide_upload reports it (a buffer of the library's own counts as 0:
 * device allocations and pinned slots are aligned far beyond 16 bytes). */
static inline uint32_t bf_ingest_copy_bytes(uint64_t in_row_bytes, uint64_t out_row_bytes, uint64_t raw, uint64_t out,
                                            uint64_t in_frame_bytes, uint64_t out_frame_bytes)
{
	uint64_t align = in_row_bytes | out_row_bytes | raw | out | in_frame_bytes | out_frame_bytes;
	return (align % 16 == 0) ? 16u : (align % 4 == 0) ? 4u : 2u;
}

typedef struct {
	const void *left, *right; void *out;
	uint32_t size[3];
	int64_t  in_stride[3], out_stride[3];
	int32_t  in_kind, out_kind, interleave;
	int64_t  in_elements;             /* elements of in_kind readable at `left` (per frame); an element past them reads as zero */
	uint32_t frames;                  /* a burst (executor.cpp push_burst): frames of the launch, 0 or 1 = one; frame f reads and writes f * the strides below further on */
	uint64_t in_frame_bytes, out_frame_bytes;
} BfReshapeArgs;

typedef struct {
	const void *in; void *out;
	const float *hadamard_t;          /* T*T floats, transposed on the host: HtT[T*i + j] = Ht[T*j + i] */
	const float *hadamard_base;       /* base*base floats B[i*base + j] when HtT = Sylvester(T/base) (x) B, else null */
	uint32_t     hadamard_base_order; /* 1, 12 or 20; 0: no such structure found, dense kernel only */
	uint32_t transmit_count, channel_count, sample_count;
	int64_t  out_stride[3];           /* sample, channel, transmit */
	int32_t  in_kind, out_kind;
	uint32_t frames;                  /* a burst (executor.cpp push_burst): frames of the launch, 0 or 1 = one; frame f reads and writes f * the strides below further on */
	uint64_t in_frame_bytes, out_frame_bytes;
} BfDecodeArgs;

typedef struct {
	const void *in; void *out;
	const float *coefficients;
	const float *phasors;             /* demodulate: {cos, -sin} of the window-local phase for index 0..D*64+L-2, or null */
	uint32_t filter_length, decimation, sample_count, batch_sample_count;
	int32_t  complex_filter, demodulate;
	float    sampling_frequency, demodulation_frequency;
	int64_t  in_stride[3], out_stride[3];
	int64_t  in_elements;
	uint32_t channels, transmits;
	int32_t  in_kind, out_kind;
	uint32_t frames;                  /* a burst (executor.cpp push_burst): frames of the launch, 0 or 1 = one; frame f reads and writes f * the strides below further on */
	uint64_t in_frame_bytes, out_frame_bytes;
} BfFilterArgs;

/* Depth-major tile walk of VOLUMES (separable gather and LDS-staged kernels).  An XCD has ~64 consecutive tiles of its run in flight (two
 * 1024-thread blocks on each of 32 CUs) and its 4 MiB L2 serves what they read.  With one column walked z fastest those are 64 consecutive
 * depths: the RF window of a (channel, transmit) drifts ~1.5 samples per plane at config 4, 96 samples over the set -- three 32-sample
 * windows apart, so most lines are pulled for one tile.  With g columns ADJACENT ALONG u walked together they are 64 / g depths (g = 4: a
 * 24-sample drift, inside one window) of columns whose transmit windows are the same and whose receive windows neighbour.  Measured on
 * config 4's staged kernel, HBM-side bytes per launch (profiles/r04_traffic.json; kernel time equal within 0.3 %): one column 288 GB,
 * g = 2 123 GB, g = 4 52 GB, g = 8 94 GB, a whole row of 16 columns 181 GB, 4 columns along v 56 GB, 2 x 2 65 GB, plane-major 96 GB.
 * The gather kernel (smaller blocks, more of them in flight, no staging loads) keeps g = 1: 280 GB against 520 with g = 4. */
static inline uint32_t bf_walk_columns(uint32_t tiles_u) { return tiles_u % 4u == 0 ? 4u : (tiles_u % 2u == 0 ? 2u : 1u); }
#ifdef __HIPCC__
static __device__ __forceinline__ void bf_column_walk(uint32_t tile, uint32_t tiles_u, uint32_t tiles_z, uint32_t g, uint32_t &tu, uint32_t &tv, uint32_t &zl)
{
	const uint32_t r = tile / g, col = r / tiles_z, per_row = tiles_u / g;
	zl = r % tiles_z;
	tu = (col % per_row) * g + tile % g;
	tv = col / per_row;
}
#endif

/* Tile walk of VIEW PLANES (depth_major == 3; depth lies along voxel y, one voxel along z -- math.c:844-885).  The work of a
 * tile grows with its depth (the f-number test culls shallow voxels), so neither a run of depth rows per XCD (idle XCDs: the
 * shallow bands finish early) nor a lateral column per XCD (an XCD's tiles in flight span half the RF rows: L2 misses x 3,
 * measured) will do.  The tile rows are cut into bands of `band_rows`; XCD k (= block id mod 8: consecutive ids land on
 * consecutive XCDs) takes bands k, 15 - k, 16 + k, 31 - k, ... -- a shallow band with a deep one -- and walks each band x
 * fastest.  Returns the number of blocks to launch. */
static inline uint32_t bf_plane_walk_blocks(uint32_t blocks_x, uint32_t blocks_y, uint32_t band_rows)
{
	uint32_t bands = (blocks_y + band_rows - 1) / band_rows;
	uint32_t slots = 2u * ((bands + 15u) / 16u);              /* bands per XCD */
	return 8u * slots * band_rows * blocks_x;
}
/* Blocks to launch for a tile walk that deals the block ids to the 8 XCDs (general_tile, das_general.h): the bands of a view plane, or
 * the tile count rounded up to a multiple of 8 -- the ids of the ragged tail have no tile. */
static inline uint32_t bf_walk_grid_blocks(uint32_t depth_major, const uint32_t blocks[3], uint32_t band_rows)
{
	const uint32_t total = blocks[0] * blocks[1] * blocks[2];
	return depth_major == 3u ? bf_plane_walk_blocks(blocks[0], blocks[1], band_rows) : ((total + 7u) / 8u) * 8u;
}
static inline uint32_t bf_general_grid_blocks(const BfDasArgs *a) { return bf_walk_grid_blocks(a->depth_major, a->blocks, a->band_rows); }
/* A channel split (BfDasArgs::split_shift, das.hip and das_factored.hip): K = 1 << split_shift waves share 64 voxels and combine
 * through [K-1][3][64] floats of LDS; without one a block is 256 threads and has no LDS. */
static inline uint32_t bf_split_threads(const BfDasArgs *a) { return a->split_shift ? 64u << a->split_shift : 256u; }
static inline uint32_t bf_split_lds_bytes(const BfDasArgs *a) { return a->split_shift ? ((1u << a->split_shift) - 1u) * 192u * (uint32_t)sizeof(float) : 0u; }
#ifdef __HIPCC__
template <bool DEEPEST_FIRST = false>
static __device__ __forceinline__ bool bf_plane_walk(uint32_t block_id, uint32_t blocks_x, uint32_t blocks_y, uint32_t band_rows,
                                                     uint32_t &bx, uint32_t &by)
{
	const uint32_t xcd = block_id & 7u, j = block_id >> 3;
	const uint32_t per_band = band_rows * blocks_x;
	uint32_t slot = j / per_band;
	const uint32_t r = j - slot * per_band;
	if constexpr (DEEPEST_FIRST) {
		/* an XCD's bands deepest first: the waves that live longest start first and the launch drains over the short ones.  Measured on
		 * the reference harness's plane (profiles/r04_harness_waits.json, one box): HERCULES 20.7 -> 19.7 ms; the factored kernel's frames
		 * are within +-3 % either way (TPW slower), so only das_hercules.hip asks for it */
		const uint32_t bands = (blocks_y + band_rows - 1) / band_rows;
		slot = 2u * ((bands + 15u) / 16u) - 1u - slot;
	}
	const uint32_t band = 16u * (slot >> 1) + ((slot & 1u) ? 15u - xcd : xcd);
	by = band * band_rows + r / blocks_x;
	bx = r % blocks_x;
	return by < blocks_y;
}
#endif

/* frames of a burst one Filter / Demodulate / Hilbert launch takes: they share grid y (at most 65535 blocks) with the channels */
static inline uint32_t bf_stage_frame_chunk(uint32_t channels) { return channels && channels < 65535u ? 65535u / channels : 1u; }

/* ---- frame metrics (frame_metrics.hip: beamformer_hip_score_last_frames) ---- */
#define BF_METRICS_MAX_BLOCKS       1024u
#define BF_METRICS_VOXELS_PER_BLOCK 1024u     /* 256 threads, four voxels each, until BF_METRICS_MAX_BLOCKS blocks walk further */
/* blocks that walk a box of `volume` voxels: a function of the box alone -- a frame's bits do not depend on its company in the launch */
static inline uint32_t bf_metrics_blocks(uint64_t volume)
{
	const uint64_t blocks = (volume + BF_METRICS_VOXELS_PER_BLOCK - 1u) / BF_METRICS_VOXELS_PER_BLOCK;
	return blocks > BF_METRICS_MAX_BLOCKS ? BF_METRICS_MAX_BLOCKS : blocks ? (uint32_t)blocks : 1u;
}
typedef struct {
	uint64_t offset;             /* of the frame in the frame ring, bytes */
	uint32_t points[3], cplx;    /* the frame's grid; 1: Float32Complex, 0: Float32 */
	uint32_t first[3], count[3]; /* the box, inside the grid, every count >= 1 */
	uint32_t blocks;             /* bf_metrics_blocks of the box */
	uint32_t partial_first;      /* its first BfMetricsPartial */
	uint32_t step[3];            /* blocks * 256 voxels of the box as steps in x, y, z: (n % cx, n / cx % cy, n / (cx * cy)) */
	uint32_t reserved;
} BfMetricsRow;
typedef struct {                 /* one block's share of a box */
	double   s1, s2, s4, g[3];
	uint64_t max_index;          /* flat index in the FRAME of the largest finite magnitude; max_abs -1: the block saw none */
	float    max_abs;
	uint32_t n, bad, pairs[3];
} BfMetricsPartial;
typedef struct {                 /* a frame's box */
	double   s1, s2, s4, g[3];
	uint64_t voxels, bad, pairs[3];
	uint64_t max_index;          /* 0 with max_abs 0 when no voxel of the box is finite */
	float    max_abs;
	uint32_t reserved;
} BfMetricsResult;

/* ---- frame peaks (frame_peaks.hip: beamformer_hip_find_peaks_last_frames) ---- */
#define BF_PEAKS_MAX_BLOCKS 0x7FFFFFFFu      /* grid x: a frame's blocks are ceil(waves / 4), uncapped (512^3: about 5 x 10^5) */
typedef struct {
	uint64_t offset;             /* of the frame in the frame ring, bytes */
	uint64_t wave_first;         /* its first 64-bit peak mask: one a wave */
	uint64_t block_first;        /* its first block count and block offset */
	uint32_t points[3], cplx;    /* the frame's grid; 1: Float32Complex, 0: Float32 */
	uint32_t first[3], count[3]; /* the box, inside the grid, every count >= 1 */
	uint32_t waves_per_row;      /* ceil(count[0] / 64): a wave owns 64 consecutive x of one box row */
	uint32_t waves, blocks;      /* waves_per_row * count[1] * count[2], in flat box order; ceil(waves / 4) */
	float    threshold;          /* on the decision value: the caller's threshold (real frames), its float32 square (complex ones) */
	uint32_t cap;                /* records kept: the first `cap` in flat order */
	uint32_t reserved;
} BfPeaksRow;
typedef struct { uint64_t found, above_threshold; } BfPeaksResult;   /* a frame's box */
/* the localisation map (frame_peaks.hip: beamformer_hip_accumulate_peaks_last_frames, beamformer_hip_queue_localisation_map) */
#define BF_MAP_MAX_VOXELS (1ull << 28)       /* = BEAMFORMER_HIP_MAX_MAP_VOXELS */
typedef struct {
	uint32_t points[3];          /* the map's grid, x fastest */
	uint32_t use_offsets;        /* 0: a peak's position is its index */
} BfMapArgs;
/* peak pairs and the track map (frame_tracks.hip: beamformer_hip_pair_peaks_last_frames, beamformer_hip_queue_track_map) */
#define BF_TRACK_MAX_VOXELS (1ull << 26)     /* = BEAMFORMER_HIP_MAX_TRACK_MAP_VOXELS */
#define BF_TRACK_MAX_PEAKS  65536u           /* = BEAMFORMER_HIP_MAX_PEAKS_PER_FRAME: records a frame */
#define BF_TRACK_NONE       0xFFFFFFFFu      /* f(a) or g(b): nothing within reach */
#define BF_TRACK_FIXED      1048576.0        /* the sums' fixed point: 2^20 a map voxel */
#define BF_TRACK_COMPONENTS 5u               /* = BEAMFORMER_HIP_TRACK_MAP_COMPONENTS */
typedef struct { uint32_t pairs, deposited, outside, reserved; } BfTrackTally;   /* a frame pair */
typedef struct {
	uint32_t points[3];          /* the track map's grid, x fastest (read with deposit only) */
	uint32_t deposit;            /* 0: nothing is added to the map */
} BfTrackArgs;
/* peak tracks (frame_tracks.hip: beamformer_hip_track_peaks_last_frames) */
#define BF_CHAIN_POINTS 1u                   /* = BEAMFORMER_HIP_TRACK_DEPOSIT_POINTS */
#define BF_CHAIN_LINKS  2u                   /* = BEAMFORMER_HIP_TRACK_DEPOSIT_LINKS */
typedef struct {                             /* a frame: BeamformerHipTrackedFrame's eight counters, in its order */
	uint32_t heads, kept_heads, kept_points, kept_links, points_deposited, points_outside, links_deposited, links_outside;
} BfChainTally;
typedef struct {
	uint32_t point_map[3];       /* the localisation map's grid, x fastest (read with BF_CHAIN_POINTS only) */
	uint32_t track_map[3];       /* the track map's (read with BF_CHAIN_LINKS only) */
	uint32_t deposit;            /* BF_CHAIN_POINTS | BF_CHAIN_LINKS */
	uint32_t min_length;         /* a track is kept with at least so many peaks */
} BfChainArgs;
/* drawn tracks (frame_tracks.hip: beamformer_hip_draw_tracks_last_frames) */
#define BF_DRAW_MAX_SMOOTH  8u               /* = BEAMFORMER_HIP_MAX_TRACK_SMOOTH */
#define BF_DRAW_MAX_SAMPLES 4096.0           /* = BEAMFORMER_HIP_MAX_LINK_SAMPLES: a link of a larger extent is skipped */
typedef struct {                             /* a frame: BeamformerHipDrawnFrame's eight counters behind kept_links, in its order */
	uint32_t lone, links_skipped, samples, repeats, points_deposited, points_outside, links_deposited, links_outside;
} BfDrawTally;
typedef struct {
	uint32_t point_map[3];       /* the localisation map's grid, x fastest (read with BF_CHAIN_POINTS only) */
	uint32_t track_map[3];       /* the track map's (read with BF_CHAIN_LINKS only) */
	uint32_t deposit;            /* BF_CHAIN_POINTS | BF_CHAIN_LINKS */
	uint32_t smooth;             /* w, the moving average's half-width; 0: none, the points are drawn as they are */
} BfDrawArgs;

/* ---- frame quantiles (frame_quantiles.hip: beamformer_hip_quantiles_last_frames) ---- */
#define BF_QUANTILES_MAX       16u           /* = BEAMFORMER_HIP_MAX_QUANTILES: ranks a frame, and so distinct prefixes a digit pass */
#define BF_QUANTILES_BINS1     2048u         /* = BEAMFORMER_HIP_QUANTILE_BINS: bits 30..20 of a decision value */
#define BF_QUANTILES_BINS      1024u         /* bits 19..10, then bits 9..0 */
typedef struct {
	uint64_t offset;             /* of the frame in the frame ring, bytes */
	uint32_t points[3], cplx;    /* the frame's grid; 1: Float32Complex, 0: Float32 */
	uint32_t first[3], count[3]; /* the box, inside the grid, every count >= 1, at most 2^32 - 1 voxels */
	uint32_t blocks;             /* bf_metrics_blocks of the box */
	uint32_t step[3];            /* blocks * 256 voxels of the box as steps in x, y, z: (n % cx, n / cx % cy, n / (cx * cy)) */
} BfQuantilesRow;                /* 64 bytes */
typedef struct { uint64_t voxels, non_finite; } BfQuantilesTally;   /* a frame's box */
typedef struct {                 /* one rank of one frame: what the pick kernels carry from pass to pass, and the answer */
	uint64_t rank, below, equal; /* below: the finite voxels under the prefix so far, at the end under the value */
	uint32_t value_bits;         /* the bit pattern of q_(rank), after the third pick */
	uint32_t prefix;             /* the leading bits selected so far: 11 after the first pick, 21 after the second */
	uint32_t residual;           /* the rank inside the prefix */
	uint32_t slot;               /* which of the frame's distinct prefixes: the table the next count pass adds to for it */
} BfQuantileState;               /* 40 bytes */
typedef struct {                 /* a frame's distinct prefixes, for the count pass that follows */
	uint64_t mask;               /* bit (prefix & 63) set for every one of them: the test most voxels fail */
	uint32_t tables, reserved;   /* how many; 0: no finite voxel */
	uint32_t prefix[BF_QUANTILES_MAX];   /* unused ones 0xFFFFFFFF, no voxel's key */
} BfQuantilesPrefixes;           /* 80 bytes */
/* the count tables of a call, uint32 words zeroed by one memset: non_finite[frames] (rounded up to 16 words) | pass 1 [frames][2048] |
 * pass 2 [frames][fractions][1024] | pass 3 likewise */
static inline size_t bf_quantiles_pass1_at(uint32_t frames) { return ((size_t)frames + 15u) / 16u * 16u; }
static inline size_t bf_quantiles_pass_words(uint32_t frames, uint32_t fractions) { return (size_t)frames * fractions * BF_QUANTILES_BINS; }
static inline size_t bf_quantiles_table_words(uint32_t frames, uint32_t fractions)
{
	return bf_quantiles_pass1_at(frames) + (size_t)frames * BF_QUANTILES_BINS1 + 2u * bf_quantiles_pass_words(frames, fractions);
}

/* ---- ensemble filter (ensemble.hip: beamformer_hip_gram_last_frames, beamformer_hip_mix_last_frames) ---- */
#define BF_ENSEMBLE_MAX_FRAMES 256u          /* = BEAMFORMER_HIP_MAX_ENSEMBLE_FRAMES */
#define BF_GRAM_TILE           32u           /* frames a side of a tile of (j, k) pairs: a block of 256 threads, four pairs a thread */
#define BF_GRAM_WORD           64u           /* voxels a word of the all-finite mask, and a staged tile of voxels */
#define BF_GRAM_MAX_CHUNKS     1024u         /* chunks x tile pairs x 16 KiB of partials: at most 16 MiB up to 64 frames, 36 MiB at 256 */
#define BF_GRAM_MIN_CHUNKS     64u
#define BF_MIX_TILE            16u           /* output frames a block of the mix kernel produces: 32 accumulator VGPRs */
static inline uint32_t bf_gram_tiles(uint32_t frames) { return (frames + BF_GRAM_TILE - 1u) / BF_GRAM_TILE; }
static inline uint32_t bf_gram_tile_pairs(uint32_t frames) { const uint32_t t = bf_gram_tiles(frames); return t * (t + 1u) / 2u; }
/* The partition of a box of `volume` voxels (flat box order, x fastest) into chunks of whole mask words: a function of the box and the
 * frame count alone, so the bits of a Gram matrix depend on nothing else.  The cap: 1024 / tile pairs chunks, at least 64 -- 1024 chunks
 * up to 32 frames, 341 at 64, 64 from 160 frames on. */
static inline uint32_t bf_gram_chunk_words(uint32_t volume, uint32_t frames)
{
	const uint32_t words = (uint32_t)(((uint64_t)volume + BF_GRAM_WORD - 1u) / BF_GRAM_WORD);
	uint32_t cap = BF_GRAM_MAX_CHUNKS / bf_gram_tile_pairs(frames);
	if (cap < BF_GRAM_MIN_CHUNKS) cap = BF_GRAM_MIN_CHUNKS;
	/* four words (256 voxels) a chunk until the cap is reached */
	const uint32_t each = (words + cap - 1u) / cap;
	return each < 4u ? 4u : each;
}
typedef struct {
	uint32_t frames, cplx;       /* K; 1: Float32Complex, 0: Float32 */
	uint32_t points[3];          /* the frames' common grid */
	uint32_t first[3], count[3]; /* the box, inside the grid, every count >= 1 */
	uint32_t volume, words;      /* voxels of the box (below 2^32), ceil(volume / 64) */
	uint32_t chunk_words, chunks;/* bf_gram_chunk_words; ceil(words / chunk_words) */
	uint32_t tiles, tile_pairs;  /* bf_gram_tiles, bf_gram_tile_pairs */
} BfGramArgs;
typedef struct {
	uint32_t frames, outputs;    /* K, M */
	uint32_t cplx;
	uint32_t padded_outputs;     /* M rounded up to BF_MIX_TILE: the rows of the weight table, zero past M */
	uint64_t elements;           /* a frame's complex voxels (cplx) or floats */
	uint64_t out_offset, out_stride;   /* the first output frame in the ring, bytes; from one output to the next */
} BfMixArgs;

/* ---- slow-time autocorrelation (autocorr.hip: beamformer_hip_autocorrelate_last_frames) ---- */
#define BF_AUTOCORR_MAX_LAGS   4u            /* = BEAMFORMER_HIP_MAX_LAGS: a chain reaches 3 rows back, carried across a tile boundary */
typedef struct {
	uint32_t frames, rows;       /* K source frames, the rows of the weight table (the identity form: rows == frames) */
	uint32_t lags, cplx;         /* output frames, lag 0 first; 1: Float32Complex, 0: Float32 */
	uint64_t elements;           /* a frame's complex voxels (cplx) or floats */
	uint64_t out_offset, out_stride;   /* the lag 0 frame in the ring, bytes; from one lag to the next */
} BfAutocorrArgs;

/* ---- separable spatial filter (spatial.hip: beamformer_hip_convolve_last_frames) ---- */
#define BF_SPATIAL_MAX_TAPS    33u           /* = BEAMFORMER_HIP_MAX_SPATIAL_TAPS: a halo of 16 voxels either side */
#define BF_SPATIAL_TAP_STRIDE  96u           /* floats of an axis's row of the device tap table: BF_SPATIAL_TAP_FRONT zeros, the taps, zeros */
#define BF_SPATIAL_TAP_FRONT   16u
typedef struct {
	uint32_t frames, cplx;       /* K frames in, K out; 1: Float32Complex, 0: Float32 */
	uint32_t stage, last;        /* 0: Zero mode; 1: Normalised, the first pass (the mask is made from the source); 2: Normalised, a later pass
	                                (D is read); last: Normalised stores N / D and no D */
	uint32_t inner, extent, outer;   /* the axis: `extent` points at a stride of `inner` voxels, `outer` slices of inner * extent voxels */
	uint32_t taps;               /* odd, <= BF_SPATIAL_MAX_TAPS */
	uint64_t in_stride, out_stride;  /* bytes from one frame to the next (in_stride: without an offsets table) */
	uint64_t d_stride;           /* floats from one frame's D field to the next */
	uint32_t row_log2, row_rows, row_segments, row_groups;   /* launch geometry, filled in by bf_launch_spatial */
	uint32_t run_blocks, run_chunks;
} BfSpatialArgs;

/* ---- shift correlation (correlate.hip: beamformer_hip_correlate_last_frames) ---- */
#define BF_CORRELATE_MAX_SHIFT    16u        /* = BEAMFORMER_HIP_MAX_SHIFT */
#define BF_CORRELATE_MAX_SHIFTS   1089u      /* = BEAMFORMER_HIP_MAX_SHIFTS */
#define BF_CORRELATE_THREADS      256u
#define BF_CORRELATE_MAX_BATCHES  5u         /* ceil(1089 / 256): the shifts a thread owns when the window has more shifts than the block threads */
#define BF_CORRELATE_TILE_VOXELS  1024u      /* reference voxels a staged tile holds at most: 16 KiB of LDS */
#define BF_CORRELATE_HALO_VOXELS  4096u      /* voxels of the tile plus its halo at most: 32 KiB of LDS and 4 KiB of validity bytes */
/* The tile of a box under a window: from 32 voxels an axis (no more than the box has), the longest side halved -- z before y before x
 * among equals, so that rows stay long -- until the tile holds at most 1024 voxels and the tile plus its halo of S voxels either side at
 * most 4096.  It ends: a tile of one voxel has a halo of T <= 1089.  A function of the box and the window alone. */
static inline void bf_correlate_tile(const uint32_t count[3], const uint32_t max_shift[3], uint32_t tile[3])
{
	for (int a = 0; a < 3; a++) tile[a] = count[a] < 32u ? count[a] : 32u;
	for (;;) {
		const uint32_t voxels = tile[0] * tile[1] * tile[2];
		const uint32_t halo = (tile[0] + 2u * max_shift[0]) * (tile[1] + 2u * max_shift[1]) * (tile[2] + 2u * max_shift[2]);
		if (voxels <= BF_CORRELATE_TILE_VOXELS && halo <= BF_CORRELATE_HALO_VOXELS) return;
		int longest = 2;
		if (tile[1] > tile[longest]) longest = 1;
		if (tile[0] > tile[longest]) longest = 0;
		tile[longest] = (tile[longest] + 1u) / 2u;
	}
}
/* tiles (in flat order, x fastest) a block of the partial pass walks: at most max(16, min(64, 16384 / T)) chunks a box -- 64 up to 256
 * shifts, 16 at 1089, where an entry's partials are large and a block's work long; a box of one tile is one chunk.  A function of the
 * box and the window alone: NOT of the frame count. */
static inline uint32_t bf_correlate_chunk_tiles(uint32_t tiles, uint32_t shifts)
{
	uint32_t cap = 16384u / shifts;
	cap = cap < 16u ? 16u : cap > 64u ? 64u : cap;
	return (tiles + cap - 1u) / cap;
}
/* voxel groups of a block: floor(256 / T) groups of T threads share a tile's voxels (group g takes the voxels n = g, g + G, ...); one
 * group from 129 shifts on */
static inline uint32_t bf_correlate_groups(uint32_t shifts) { return shifts < BF_CORRELATE_THREADS ? BF_CORRELATE_THREADS / shifts : 1u; }
typedef struct {                 /* one box of a call */
	uint32_t first[3], count[3]; /* inside the frames' grid, every count >= 1 */
	uint32_t tile[3];            /* bf_correlate_tile */
	uint32_t tiles[3];           /* ceil(count / tile) an axis */
	uint32_t halo[3];            /* tile + 2 S */
	uint32_t tile_voxels, halo_voxels;
	uint32_t chunk_tiles, chunks;/* bf_correlate_chunk_tiles; ceil(tiles / chunk_tiles) */
	uint32_t reserved;
	uint64_t partial_first;      /* its first BfCorrelateEntry among the partials: [chunk][frame][shift] from there */
} BfCorrelateRow;
typedef struct { double re, im, energy_reference, energy_frame; uint64_t terms; } BfCorrelateEntry;   /* = BeamformerHipShiftCorrelation */
typedef struct {
	uint32_t frames, reference;  /* K; the reference's index among them */
	uint32_t cplx, regions;      /* 1: Float32Complex, 0: Float32; R */
	uint32_t points[3];          /* the frames' common grid */
	uint32_t max_shift[3];       /* S */
	uint32_t window[3];          /* 2 S + 1 */
	uint32_t shifts;             /* T */
	uint32_t groups, batches;    /* bf_correlate_groups; ceil(T / 256) */
	uint32_t max_chunks;         /* the most chunks any row has: grid x */
	uint32_t reserved;
} BfCorrelateArgs;

/* ---- warp (warp.hip: beamformer_hip_warp_last_frames) ---- */
#define BF_WARP_THREADS     256u             /* lanes, and output voxels, of a block: a tile of 2^tile_log2[a] voxels an axis */
#define BF_WARP_BOX_VOXELS  4096u            /* the staged path's LDS budget: source voxels a block stages (32 KiB complex, 16 KiB real) */
#define BF_WARP_MAX_NODES   4096u            /* = BEAMFORMER_HIP_MAX_WARP_NODES */
#define BF_WARP_MAX_ENTRIES 32768u           /* = BEAMFORMER_HIP_MAX_WARP_ENTRIES */
typedef struct {
	uint32_t frames, cplx;       /* K frames in, K out; 1: Float32Complex, 0: Float32 */
	uint32_t cubic, clamp;       /* BeamformerHipWarpInterpolation, BeamformerHipWarpEdge */
	uint32_t rotate;             /* 1: the table's rotations are applied */
	uint32_t direct;             /* 1: every tile takes the direct path (measurements and tests; the bytes are the same) */
	uint32_t points[3];          /* the frames' common grid */
	uint32_t nodes[3];           /* N_a */
	float    node_first[3], inv_step[3];   /* (not read where N_a == 1) */
	uint64_t out_offset, out_stride;       /* output n at ring + out_offset + n * out_stride */
	uint32_t tile_log2[3], tiles[3];       /* launch geometry, filled in by bf_launch_warp */
} BfWarpArgs;
/* the call's flat table: rotations[frames][2] | field[frames][nodes z][nodes y][nodes x][3] */
static inline uint32_t bf_warp_table_floats(uint32_t frames, uint32_t node_product) { return frames * 2u + frames * node_product * 3u; }
/* the tile of a grid: at most 256 voxels, the eight bits dealt round-robin, x first, over the axes whose tile does not yet cover the
 * axis (8 x 8 x 4 in a volume, 16 x 16 on a plane, 256 along a line; 2 x 1 x N: 2 x 1 x 128; 1 x 1 x 1: one voxel).  Bits that no axis
 * can take stay undealt: the lanes beyond the tile's voxels idle */
static inline void bf_warp_tile(const uint32_t points[3], uint32_t tile_log2[3])
{
	uint32_t bits = 8, idle = 0, a = 0;
	for (uint32_t k = 0; k < 3; k++) tile_log2[k] = 0;
	while (bits && idle < 3u) {
		if ((1u << tile_log2[a]) < points[a]) { tile_log2[a]++; bits--; idle = 0; } else idle++;
		a = (a + 1u) % 3u;
	}
}

/* ---- block-wise ensemble filter (ensemble_blocks.hip: beamformer_hip_gram_boxes_last_frames, beamformer_hip_mix_field_last_frames) ---- */
#define BF_BLOCKS_MAX_BOXES    1024u         /* = BEAMFORMER_HIP_MAX_GRAM_BOXES */
#define BF_BLOCKS_BUDGET       (64ull << 20) /* bytes of partials a batch of boxes may hold (hook GRAM_BOXES_BUDGET sets another) */
#define BF_BLEND_MAX_NODES     1024u         /* = BEAMFORMER_HIP_MAX_MIX_NODES */
#define BF_BLEND_MAX_ENTRIES   (1u << 22)    /* = BEAMFORMER_HIP_MAX_MIX_FIELD_ENTRIES */
/* one box of a batch: the arguments the single-box kernels take -- the chunking is the box's own bf_gram_chunk_words --, and where the
 * box's blocks, mask words, partials and result lie in the batch */
typedef struct {
	BfGramArgs a;
	uint32_t mask_block_first;   /* the box's first block of the mask pass (ceil(words / 4) blocks a box), a prefix over the batch */
	uint32_t partial_block_first;/* ... of the partial pass (chunks x tile pairs blocks a box, the tile pair fastest) */
	uint64_t mask_first;         /* the box's first word in the batch's mask */
	uint64_t partial_first;      /* its first (chunk, tile pair) in the batch's partials */
	uint64_t result_first;       /* its result {voxels, non_finite, gram[frames][frames][2]} in the call's results, bytes */
} BfBlocksBox;
/* one segment cell of the field mix: a box of the frame whose voxels share their (up to) 8 corner nodes */
typedef struct {
	uint32_t first[3], count[3]; /* the box, inside the frame, every count >= 1; a voxel's r along axis a is its index inside the box */
	uint32_t node[3];            /* the lower node along each axis */
	uint32_t corners[3];         /* 2: nodes node[a] and node[a] + 1 are blended along axis a; 1: node[a] alone */
	uint32_t volume;             /* voxels of the box */
	uint32_t block_first;        /* the cell's first block (ceil(volume / 256) x output tiles blocks a cell, the tile fastest), a prefix */
	uint32_t reserved[2];
} BfBlendCell;
typedef struct {
	uint32_t frames, outputs;    /* K, M */
	uint32_t cplx;
	uint32_t padded_outputs;     /* M rounded up to BF_MIX_TILE: the rows of a node's weight table, zero past M */
	uint32_t points[3];          /* the frames' common grid */
	uint32_t nodes[3];           /* N_a */
	float    inv_step[3];        /* 1.0f / node_step[a] (not read where N_a == 1) */
	uint32_t cells, blocks;      /* cells of the table, blocks of the launch */
	uint32_t once;               /* 1: blend_once_kernel, each source loaded once a k for all corners (nodes[1] == 1 only; the bytes are the same) */
	uint32_t reserved;
	uint64_t out_offset, out_stride;   /* the first output frame in the ring, bytes; from one output to the next */
} BfBlendArgs;

#ifdef __cplusplus
extern "C" {
#endif
/* every launcher returns the hipError_t of the launch; nothing synchronises */
hipError_t bf_launch_ingest(const BfIngestArgs *a, hipStream_t s);
hipError_t bf_launch_reshape(const BfReshapeArgs *a, hipStream_t s);
hipError_t bf_launch_decode(const BfDecodeArgs *a, hipStream_t s);
hipError_t bf_launch_filter(const BfFilterArgs *a, hipStream_t s);
hipError_t bf_launch_hilbert(const BfFilterArgs *a, hipStream_t s);
hipError_t bf_launch_das(const BfDasArgs *a, hipStream_t s);
hipError_t bf_launch_das_count(const BfDasArgs *a, hipStream_t s);
hipError_t bf_launch_das_burst(const BfDasArgs *a, const BfBurstArgs *b, hipStream_t s);   /* das_burst.hip: RCA family, `a` without a channel split */
hipError_t bf_launch_das_readi_sweep(const BfDasArgs *a, const BfReadiSweepArgs *b, hipStream_t s);   /* das_burst.hip: READI, `a` without a channel split */
hipError_t bf_launch_readi_image_decode(const BfReadiDecodeArgs *a, hipStream_t s);   /* readi_decode.hip */
hipError_t bf_launch_views_table(void *dst, const void *src, uint32_t bytes, hipStream_t s);   /* das_views.hip: bytes (a multiple of 4) from mapped pinned memory into the device table */
hipError_t bf_launch_das_views(const BfDasArgs *a, const BfViewsArgs *v, uint32_t total_blocks, hipStream_t s);   /* das_views.hip: RCA family, no channel split */
/* das_burst.hip: the burst kernel's frame slots on the views kernel's tiles -- RCA family, no channel split; frame f of the view of row r
 * reads a->rf + f * b->rf_stride and writes a->out + r.out_offset + f * r.out_stride (b->out_stride is not read) */
hipError_t bf_launch_das_burst_views(const BfDasArgs *a, const BfBurstArgs *b, const BfViewsArgs *v, uint32_t total_blocks, hipStream_t s);
/* das_variants.hip: RCA family, 256-voxel tiles in a walk order general_tile_at knows (depth_major 0 - 2), no channel split, the whole
 * grid; variant r of the launch runs under rows[r] (device) and writes a->out + rows[r].out_offset */
hipError_t bf_launch_das_variants(const BfDasArgs *a, const BfVariantRow *rows, uint32_t variant_count, hipStream_t s);
hipError_t bf_launch_das_separable(const BfDasArgs *a, const BfSeparableArgs *q, hipStream_t s);
hipError_t bf_launch_das_staged(const BfDasArgs *a, const BfSeparableArgs *q, hipStream_t s);
hipError_t bf_launch_das_staged_tables(const BfDasArgs *a, const BfSeparableArgs *q, hipStream_t s);
hipError_t bf_launch_das_staged_real(const BfDasArgs *a, const BfSeparableArgs *q, hipStream_t s);
hipError_t bf_launch_das_staged_cubic(const BfDasArgs *a, const BfSeparableArgs *q, hipStream_t s);
/* |v| (complex) or v (real) min/max over a frame -> out2 (device float[2]); scratch holds
 * 2*1024 floats */
hipError_t bf_launch_das_factored(const BfDasArgs *a, hipStream_t s);
hipError_t bf_launch_das_tile(const BfDasArgs *a, hipStream_t s);          /* das_tile.hip: the factored kernel with block-wide LDS staging (cubic IQ, fine grids) */
hipError_t bf_launch_das_hercules(const BfDasArgs *a, const BfHerculesArgs *q, hipStream_t s);
hipError_t bf_launch_sum(void *out, const void *in, float prescale, uint64_t bytes, hipStream_t s);
hipError_t bf_launch_display(const void *frame, uint64_t voxels, int complex_data, float threshold_db,
                             float gamma, float db_cutoff, float *out, hipStream_t s);
hipError_t bf_launch_min_max(const void *frame, uint64_t voxels, int complex_data,
                             float *scratch, float *out2, hipStream_t s);
/* frame_metrics.hip: two launches, no atomics -- a partial pass (grid x max_blocks, the most blocks any row asks for; grid y the frame) and
 * one wave a frame that folds its partials into results[frame].  `ring` and the three tables are device memory; every row's box lies
 * inside its frame (the caller checks: the kernels index with what the rows say) */
hipError_t bf_launch_frame_metrics(const void *ring, const BfMetricsRow *rows, uint32_t frame_count, uint32_t max_blocks,
                                   BfMetricsPartial *partials, BfMetricsResult *results, hipStream_t s);
/* frame_quantiles.hip: one memset and six launches -- three count passes (grid x max_blocks, the most blocks any row asks for; grid y the
 * frame), each followed by a pick, one block a frame.  `tables`: bf_quantiles_table_words(frame_count, fraction_count) words, zeroed
 * here; fractions[fraction_count]; prefixes[frame_count]; tallies[frame_count]; states[frame_count][fraction_count].  Integer atomics
 * only.  All tables are device memory; every row's box lies inside its frame and holds at most 2^32 - 1 voxels (the caller checks: the
 * kernels index with what the rows say) */
hipError_t bf_launch_frame_quantiles(const void *ring, const BfQuantilesRow *rows, const double *fractions, uint32_t frame_count,
                                     uint32_t fraction_count, uint32_t max_blocks, uint32_t *tables, BfQuantilesPrefixes *prefixes,
                                     BfQuantilesTally *tallies, BfQuantileState *states, hipStream_t s);
/* frame_peaks.hip: three launches, no atomics.  _mark: the mark pass (grid x max_blocks, the most blocks any row asks for; grid y the
 * frame) and the scan, one block a frame; _emit: the mark pass's grid again, storing 32-byte records (BeamformerHipFramePeak's layout) at
 * list[firsts[frame] + rank].  The host reads `results` between the two to size `list` and to fill `firsts`.  All tables are device
 * memory; every row's box lies inside its frame (the caller checks: the kernels index with what the rows say) */
hipError_t bf_launch_frame_peaks_mark(const void *ring, const BfPeaksRow *rows, uint32_t frame_count, uint32_t max_blocks,
                                      uint64_t *masks, uint32_t *counts, uint32_t *offsets, BfPeaksResult *results, hipStream_t s);
hipError_t bf_launch_frame_peaks_emit(const void *ring, const BfPeaksRow *rows, uint32_t frame_count, uint32_t max_blocks,
                                      const uint64_t *masks, const uint32_t *counts, const uint32_t *offsets, const uint32_t *firsts,
                                      void *list, hipStream_t s);
/* frame_peaks.hip, the localisation map.  _deposit: two launches behind _mark's, on its tables -- the mark pass's grid again, every peak
 * placed through placements[frame][12] (row-major 3 x 4, double) and added to its bin of `map` (uint32, a->points voxels) by one integer
 * atomic, a word a block (deposited | outside << 16) into `words`; then the scan kernel over those words: tallies[frame].found the
 * frame's deposited peaks, .above_threshold the ones outside the map (`offsets` is rewritten).  bf_launch_localisation_convert: one launch,
 * out[i] = (float)map[i] * scale */
hipError_t bf_launch_localisation_deposit(const void *ring, const BfPeaksRow *rows, const double *placements, uint32_t frame_count,
                                         uint32_t max_blocks, const uint64_t *masks, const uint32_t *counts, uint32_t *offsets,
                                         const BfMapArgs *a, uint32_t *map, uint32_t *words, BfPeaksResult *tallies, hipStream_t s);
hipError_t bf_launch_localisation_convert(const uint32_t *map, float *out, uint64_t voxels, float scale, hipStream_t s);
/* frame_tracks.hip, behind bf_launch_frame_peaks_emit on the same stream: frame n's stored[n] records lie at list[firsts[n]] (firsts,
 * stored: device memory, `frames` entries; max_stored, the most records of one frame, sizes the grids).  _place: one launch, three
 * doubles a record into `positions` (NaN: unplaced) and the frames' unplaced counts (zeroed by the caller, integer atomics).  _nearest,
 * the hot kernel: one launch, grid (blocks of 256 queries, frame pair, direction); forward[firsts[n] + a] = f(a) and
 * backward[firsts[n + 1] + b] = g(b) of frame pair n, BF_TRACK_NONE for none; stored[n] x stored[n + 1] distance evaluations a
 * direction.  _pair: three launches (match, scan, emit); block_firsts[frames - 1]: frame pair n's first block of ceil(stored[n] / 256),
 * `blocks` in all; masks: four words a block; words, offsets: one a block; tallies[frames - 1], zeroed by the caller; pairs: NULL, or
 * 48-byte records (BeamformerHipPeakPair's layout) PACKED, frame pair after frame pair, at most the sum of min(stored[n], stored[n + 1]);
 * with t->deposit the track map: map_counts, the grid's voxels of uint32, map_sums, three times as many int64 (integer atomics).
 * bf_launch_track_convert: one launch, a frame of the map's grid from counts and sums (min_pairs 0 counts as 1) */
hipError_t bf_launch_tracks_place(const void *list, const double *placements, const uint32_t *firsts, const uint32_t *stored,
                                  uint32_t frames, uint32_t max_stored, uint32_t use_offsets, double *positions, uint32_t *unplaced, hipStream_t s);
hipError_t bf_launch_tracks_nearest(const double *positions, const uint32_t *firsts, const uint32_t *stored, uint32_t frames,
                                    uint32_t max_stored, double r2, uint32_t *forward, uint32_t *backward, hipStream_t s);
hipError_t bf_launch_tracks_pair(const double *positions, const uint32_t *firsts, const uint32_t *stored, const uint32_t *block_firsts,
                                 uint32_t frames, uint32_t max_stored, uint32_t blocks, const uint32_t *forward, const uint32_t *backward,
                                 uint64_t *masks, uint32_t *words, uint32_t *offsets, const BfTrackArgs *t, uint32_t *map_counts,
                                 void *map_sums, void *pairs, BfTrackTally *tallies, hipStream_t s);
hipError_t bf_launch_track_convert(const uint32_t *counts, const void *sums, float *out, uint64_t voxels, uint32_t component,
                                   uint32_t min_pairs, float scale, hipStream_t s);
/* frame_tracks.hip, behind _nearest on the same stream: the pairs chained into tracks, ceil(log2(frames)) + 5 launches (link, the
 * pointer-jumping rounds, keep, the scan twice, finish), integer work but for the displacements.  total: the records of all frames,
 * at most 2^26.  forward, backward: _nearest's, or both NULL when it did not run (no frame pair with peaks on both sides: no links).
 * Tables of the caller's, unread before they are written here: next, lengths, tails, track_of, first_of: `total` uint32 each; links:
 * 2 x total pairs of uint32 (8-byte aligned); words, offsets: 2 x ceil(total / 256) uint32 each.  tracks, points: NULL, or room for
 * `total` records of BeamformerHipPeakTrack's and BeamformerHipTrackPoint's layout (8-byte aligned), written PACKED in the order of the
 * definition.  With a->deposit & BF_CHAIN_POINTS: point_map, a->point_map voxels of uint32; with BF_CHAIN_LINKS: track_counts and
 * track_sums as _pair takes them, a->track_map voxels.  tallies[frames]: zeroed by the caller (integer atomics, a wave a counter) */
hipError_t bf_launch_tracks_chain(const double *positions, const uint32_t *firsts, const uint32_t *stored, uint32_t frames, uint32_t max_stored,
                                  uint32_t total, const uint32_t *forward, const uint32_t *backward, uint32_t *next, void *links, uint32_t *lengths,
                                  uint32_t *tails, uint32_t *track_of, uint32_t *first_of, uint32_t *words, uint32_t *offsets, const BfChainArgs *a,
                                  uint32_t *point_map, uint32_t *track_counts, void *track_sums, void *tracks, void *points, BfChainTally *tallies,
                                  hipStream_t s);
/* frame_tracks.hip, behind _chain on the same stream and on ITS tables (links, lengths, track_of, first_of, words, offsets: as they
 * were passed to it; tracks, points: not NULL here): the kept tracks drawn into the maps, one launch (draw), two with a->smooth (smooth,
 * draw).  smoothed: room for 3 x total doubles (not read or written with a->smooth == 0).  The maps as _chain takes them.
 * tallies[frames]: zeroed by the caller (integer atomics, a wave a counter) */
hipError_t bf_launch_tracks_draw(const uint32_t *firsts, const uint32_t *stored, uint32_t frames, uint32_t max_stored, uint32_t total,
                                 const void *links, const uint32_t *lengths, const uint32_t *track_of, const uint32_t *first_of,
                                 const uint32_t *words, const uint32_t *offsets, const void *tracks, const void *points, double *smoothed,
                                 const BfDrawArgs *a, uint32_t *point_map, uint32_t *track_counts, void *track_sums, BfDrawTally *tallies,
                                 hipStream_t s);
/* ensemble.hip, the Gram matrix: three launches, no atomics -- the all-finite mask (a wave a word of 64 box voxels, every frame read
 * once), the partial pass (grid x the chunk, grid y the tile pair: BF_GRAM_TILE x BF_GRAM_TILE pairs of double2 a block) and the fold
 * (a thread a pair j <= k sums its chunks' partials in chunk order and stores both triangles; one more block counts the mask's bits).
 * offsets[frames]: where each frame lies in the ring, bytes, oldest first.  result: {uint64 voxels, uint64 non_finite, double
 * gram[frames][frames][2]}.  All tables are device memory; the box lies inside every frame (the caller checks) */
hipError_t bf_launch_gram(const void *ring, const uint64_t *offsets, const BfGramArgs *a, uint64_t *mask, double *partials, void *result, hipStream_t s);
/* ensemble.hip, the mix: one launch.  weights[padded_outputs][frames][2] floats (real frames: the imaginary ones are not read) and
 * offsets[frames] are device memory; output j is written at ring + out_offset + j * out_stride */
hipError_t bf_launch_mix(void *ring, const uint64_t *offsets, const float *weights, const BfMixArgs *a, hipStream_t s);
/* ensemble_blocks.hip, the Gram matrices of one batch of boxes: the three passes of bf_launch_gram, each ONE launch over all boxes of
 * the batch.  host_boxes: the batch's rows as the caller filled them (read here for the launch shapes and checked as bf_launch_gram
 * checks its arguments), boxes: the same rows in device memory; mask_blocks, partial_blocks: the batch's totals.  mask, partials: the
 * batch's own (a box's rows say where in them it lies); results: the call's.  The boxes lie inside every frame (the caller checks) */
hipError_t bf_launch_gram_boxes(const void *ring, const uint64_t *offsets, const BfBlocksBox *host_boxes, const BfBlocksBox *boxes, uint32_t box_count,
                                uint32_t mask_blocks, uint32_t partial_blocks, uint64_t *mask, double *partials, void *results, hipStream_t s);
/* ensemble_blocks.hip, the field mix: one launch.  weights[node][padded_outputs / BF_MIX_TILE][frames][BF_MIX_TILE][2] floats -- a mix's
 * table a node, in the lattice's flat node order --, cells[a->cells] and offsets[frames] are device memory; the cells tile the frame, and
 * a->blocks is the sum their block_first prefix ends in (the caller builds both: frame_ops.cpp) */
hipError_t bf_launch_blend(void *ring, const uint64_t *offsets, const float *weights, const BfBlendCell *cells, const BfBlendArgs *a, hipStream_t s);
/* autocorr.hip: one launch.  weights: the mix's table of `rows` rows, [ceil(rows / BF_MIX_TILE)][frames][BF_MIX_TILE][2] floats, rows past
 * `rows` zero -- or NULL, the identity form (rows == frames: row n is source frame n).  Lag l is written at ring + out_offset +
 * l * out_stride */
hipError_t bf_launch_autocorr(void *ring, const uint64_t *offsets, const float *weights, const BfAutocorrArgs *a, hipStream_t s);
/* spatial.hip: one pass along one axis, one launch.  Frame k is read at in + offsets[k] (offsets: device memory) or, offsets NULL, at
 * in + k * in_stride, and written at out + k * out_stride; taps: the axis's taps inside their row of the device table, readable from
 * taps[-BF_SPATIAL_TAP_FRONT] to the row's end; d_in / d_out: the D fields of a Normalised
 * pass, frame k at k * d_stride floats (d_in: stage 2; d_out: stages 1 and 2 unless `last`) */
hipError_t bf_launch_spatial(const void *in, const uint64_t *offsets, void *out, const float *d_in, float *d_out, const float *taps,
                             const BfSpatialArgs *a, hipStream_t s);
/* correlate.hip: two launches, no atomics -- the partial pass (grid x the chunk of a box's tiles, y the frame, z the region: one
 * BfCorrelateEntry a shift a block) and the fold (a thread an entry of the table sums its chunks' partials in chunk order).
 * offsets[frames]: where each frame lies in the ring, bytes, oldest first; rows[regions]; table[regions][frames][shifts].  All tables are
 * device memory; every row's box lies inside the frames and its geometry is what the functions above give (the caller's business) */
hipError_t bf_launch_correlate(const void *ring, const uint64_t *offsets, const BfCorrelateRow *rows, const BfCorrelateArgs *a,
                               BfCorrelateEntry *partials, BfCorrelateEntry *table, hipStream_t s);
/* warp.hip: one launch.  Source n is read at ring + offsets[n] (offsets: device memory), output n written at ring + out_offset +
 * n * out_stride; table: bf_warp_table_floats floats of device memory.  The frames hold at most 2^31 - 1 voxels, every field value
 * is finite and of magnitude <= BEAMFORMER_HIP_MAX_WARP_DISPLACEMENT (the caller checks: the kernel converts positions to indices) */
hipError_t bf_launch_warp(void *ring, const uint64_t *offsets, const float *table, const BfWarpArgs *a, hipStream_t s);
/* out (device) = sum over the 8-byte words w[i] of the buffer of w[i] * (i + 1) mod 2^64 */
hipError_t bf_launch_rf_checksum(const void *data, uint64_t bytes, unsigned long long *out, hipStream_t s);
#ifdef __cplusplus
}
#endif
#endif
