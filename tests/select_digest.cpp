/* select_digest.cpp -- every decision csrc/das_select.cpp takes for a fixed lattice of parameter blocks, printed field by field and
 * hashed, CPU only: the net under a change to the selection that is meant to change no decision.  Uses only the entry points of
 * das_select.h.  A RUN is one block under one das path mode (and at most one hook); its text holds decide_das_parts, decide_burst (plain
 * and sweep), decide_views and decide_burst_views on two view lists, decide_variants (below and at kVariantsMinVariants, with and without
 * `known`) and, for READI blocks, derive_readi_image + decide_readi_image.  Floats are printed as their bits.
 *   select_digest             one line per run: id, path of every part, part count, FNV-1a 64 of the run's text (tests/golden/das_select_digest.txt)
 *   select_digest --full      the whole text: a deliberate change of a rule shows which runs moved, and in what
 *   select_digest --coverage  what the lattice reached
 * Exit 2 unless the lattice reached every item of the coverage table (main): a condition on the inputs.
 * Built and run by tests/test_select_digest.py. */
#include "../ogl_beamforming_amd/csrc/das_select.cpp"
#include "../ogl_beamforming_amd/csrc/planner.cpp"
#include "../ogl_beamforming_amd/csrc/host_math.cpp"

#include <map>
#include <type_traits>

using namespace bf;

/* ---------------------------------------------------------------- the text of a run */

static std::string T;

static void hex(uint64_t v)
{
	char b[17]; int n = 0;
	do { b[n++] = "0123456789abcdef"[v & 15]; v >>= 4; } while (v);
	while (n) T += b[--n];
}
template <typename V> static void put(const char *name, V v)
{
	T += name; T += '=';
	if constexpr (std::is_same<V, float>::value) { uint32_t bits; std::memcpy(&bits, &v, 4); T += 'f'; hex(bits); }
	else if constexpr (std::is_same<V, bool>::value) hex(v ? 1 : 0);
	else hex((uint64_t)(typename std::make_unsigned<V>::type)v);
	T += ' ';
}
template <typename V, size_t N> static void puta(const char *name, const V (&v)[N])
{
	T += name; T += "=[";
	for (size_t i = 0; i < N; i++) {
		if constexpr (std::is_same<V, float>::value) { uint32_t bits; std::memcpy(&bits, &v[i], 4); hex(bits); }
		else hex((uint64_t)(typename std::make_unsigned<V>::type)v[i]);
		T += i + 1 < N ? ',' : ']';
	}
	T += ' ';
}
static void put(const char *name, const std::string &s) { T += name; T += "=\""; T += s; T += "\" "; }
static void open(const char *name)  { T += name; T += "{ "; }
static void close()                 { T += "} "; }
#define P(s, f) put(#f, (s).f)
#define PA(s, f) puta(#f, (s).f)

static void dump(const char *name, const BfDasArgs &a)
{
	open(name);
	PA(a, xdc_transform); PA(a, voxel_transform); PA(a, pitch);
	P(a, family); P(a, interpolation); P(a, complex_data); P(a, coherency_weighting);
	P(a, acquisition_count); P(a, channel_count); P(a, sample_count); P(a, sparse);
	P(a, sampling_frequency); P(a, inv_sampling_frequency); P(a, demodulation_frequency);
	P(a, inv_speed_of_sound); P(a, time_offset); P(a, f_number); P(a, speed_of_sound); P(a, turns_per_sample); P(a, first_transmit_weight);
	PA(a, size); P(a, z_first); P(a, z_count); P(a, readi_group_count); P(a, readi_group);
	PA(a, tile_shift); P(a, split_shift); PA(a, blocks); P(a, depth_major); P(a, band_rows); P(a, zero_offset); P(a, tile_window_shift);
	P(a, edge_margin); P(a, row_ends);
	close();
}
static void dump(const char *name, const BfSeparableArgs &q)
{
	open(name);
	P(q, u_axis); P(q, u_shift); P(q, v_shift); P(q, threads); P(q, channel_chunk); P(q, lds_bytes); PA(q, tiles); P(q, depth_major);
	P(q, walk_columns); P(q, window_shift); P(q, zero_offset); P(q, uniform); P(q, window_samples); P(q, table_stride);
	close();
}
static void dump(const char *name, const BfHerculesArgs &q)
{
	open(name);
	P(q, table_pitch); P(q, inner_count); P(q, outer_count); P(q, inner_coord); P(q, inner_is_transmit); PA(q, tiles); P(q, rows);
	P(q, depth_major); P(q, band_rows); P(q, zero_offset); P(q, unit_scale2); P(q, samples_per_unit); P(q, phase_local);
	close();
}

/* ---------------------------------------------------------------- what the lattice reached */

static std::map<std::string, unsigned long> reached;
static void reach(const std::string &what) { reached[what]++; }
static bool starts(const std::string &s, const char *prefix) { return s.compare(0, std::strlen(prefix), prefix) == 0; }

static void dump(const char *name, const DasDecision &d)
{
	open(name);
	P(d, valid); P(d, generation); P(d, hooks_version); P(d, z_first); P(d, z_count); P(d, mode); P(d, mode_asked);
	dump("a", d.a);
	P(d, tile_spread); PA(d, tile_estimate_shift);
	dump("general", d.general);
	P(d, path); P(d, depth_axis);
	dump("sep", d.sep); dump("sep_gather", d.sep_gather); P(d, has_lds_tables); dump("sep_lds_tables", d.sep_lds_tables);
	dump("herc", d.herc); P(d, hercules_prepared); P(d, das_input_bytes);
	for (int k = 0; k < DasPath_Count; k++) { char w[16]; std::snprintf(w, sizeof w, "why%d", k); put(w, d.why[k]); }
	P(d, row_end_fallback);
	close();

	char path[24]; std::snprintf(path, sizeof path, "path %d", d.path); reach(path);
	if (d.path == DasPath_Staged) reach(d.sep.uniform ? "staged: global tables" : "staged: LDS tables");
	if (d.path == DasPath_Staged && d.has_lds_tables && !d.sep.uniform)      /* has_lds_tables: the first plan had global tables */
		reach("staged: the table cap sends it to the LDS-table shape");
	if (d.path == DasPath_Gather && starts(d.why[DasPath_Staged], "global transmit table too large")) reach("staged: the table cap sends it to the gather kernel");
	if (d.path == DasPath_General) reach(d.a.split_shift ? "channel split on" : "channel split off");
	if (d.path == DasPath_Tile) reach("tile: taken");
	if (starts(d.why[DasPath_Tile], "coarse grid")) reach("tile: estimated away");
	if (starts(d.why[DasPath_Tile], "das path flag 0x200")) reach("tile: forbidden");
}
static void dump(const char *name, const std::vector<DasDecision> &parts)
{
	open(name);
	put("count", parts.size());
	for (const DasDecision &d : parts) dump("part", d);
	if (!parts.empty()) { put("row_end_planes", row_end_planes(parts)); put("main_z_first", main_part(parts).z_first); }
	close();
	if (parts.size() >= 2) reach("a frame cut into parts by the row-end rule");
}
static void dump(const char *name, const BurstDecision &b)
{
	open(name);
	P(b, burst_kernel); P(b, readi_sweep); P(b, single_path); P(b, frames_per_thread); P(b, das_launches); P(b, stage_launches); P(b, min_frames);
	P(b, reason); dump("a", b.a);
	close();
	if (b.burst_kernel) reach(b.readi_sweep && b.a.family == BF_DAS_READI ? "burst: the sweep kernel taken" : "burst: taken");
	else {
		static const char *const declines[] = {"no DAS stage runs", "acquisition kind or interpolation", "das path flag 0x400", "the burst kernel exists for",
		                                       "the row-end rule cuts", "single frames run the", "fewer than"};
		for (const char *p : declines) if (starts(b.reason, p)) reach(std::string("burst declined: ") + p);
	}
}
static void dump(const char *name, const ViewsDecision &v, uint32_t view_count, bool count_it)
{
	open(name);
	put("views", v.parts.size());
	for (const auto &parts : v.parts) dump("view", parts);
	open("taken"); for (uint8_t t : v.taken) { hex(t); T += ' '; } close();
	for (const BfViewRow &r : v.rows) {
		open("row");
		PA(r, voxel_transform); PA(r, size); PA(r, tile_shift); PA(r, blocks); P(r, depth_major); P(r, band_rows); P(r, pad0); P(r, out_offset); P(r, out_stride);
		close();
	}
	open("first_block"); for (uint32_t f : v.first_block) { hex(f); T += ' '; } close();
	P(v, kernel_views); P(v, kernel_tiles); P(v, das_launches); dump("a", v.a); P(v, reason);
	close();
	if (count_it) reach(v.kernel_views == view_count ? "views: all taken" : v.kernel_views ? "views: some taken" : "views: none taken");
}
static void dump(const char *name, const BurstViewsDecision &b, uint32_t view_count)
{
	open(name);
	dump("views", b.views, view_count, false);
	P(b, rung); P(b, kernel_views); P(b, frame_kernel_views); P(b, frames_per_thread); P(b, das_launches); P(b, stage_launches); P(b, min_frames); P(b, reason);
	close();
	char rung[24]; std::snprintf(rung, sizeof rung, "burst views: rung %u", b.rung); reach(rung);
}
static void dump(const char *name, const VariantsDecision &v)
{
	open(name);
	put("variants", v.parts.size());
	for (const auto &parts : v.parts) dump("variant", parts);
	open("taken"); for (uint8_t t : v.taken) { hex(t); T += ' '; } close();
	for (const BfVariantRow &r : v.rows) {
		open("row");
		P(r, speed_of_sound); P(r, inv_speed_of_sound); P(r, time_offset); P(r, f_number); P(r, edge_margin); P(r, pad0); P(r, out_offset);
		close();
	}
	P(v, kernel_variants); P(v, kernel_tiles); P(v, das_launches); dump("a", v.a); P(v, reason);
	close();
	if (v.kernel_variants) reach(v.kernel_variants >= kVariantsMinVariants ? "variants: taken by count" : "variants: taken by tiles");
	else if (starts(v.reason, "fewer than")) reach("variants: declined below both thresholds");
}
static void dump(const char *name, const ReadiImageDecision &r)
{
	open(name);
	P(r, transmit_count); P(r, das_launches); P(r, stage_launches); P(r, decode_launches); P(r, path); P(r, reason);
	close();
	reach(r.path == -1 ? "READI image: no DAS stage" : "READI image: a DAS stage");
}

/* ---------------------------------------------------------------- the lattice */

enum Grid { Volume, PlaneXZ, PlaneYZ, Tilted };          /* Volume: axes on the array's; Plane*: a view plane, depth on voxel y; Tilted: a volume turned 10 degrees about y */
enum Stages { DasOnly, DemodulateDas, NoDas };

struct Spec {
	const char *name;
	int      kind;
	uint32_t C, A, S;
	Grid     grid;
	uint32_t points[3];
	float    lo[3], hi[3];
	float    fs = 12.5e6f, f_number = 0.6f, pitch = 0.3e-3f, angle_span = 12.f;
	bool     iq = true, cw = false, sparse = false, focused = false, mixed_orientations = false;
	int      interpolation = 1;
	uint32_t orientation = 0x12, readi_groups = 0, readi_group = 0, shard_first = 0, shard_count = 0;
	Stages   stages = DasOnly;
};

static const float LO3[3] = {-3e-3f, -3e-3f, 6e-3f}, HI3[3] = {3e-3f, 3e-3f, 18e-3f};

static Spec spec(const char *name, int kind, uint32_t C, uint32_t A, uint32_t S, Grid grid, uint32_t px, uint32_t py, uint32_t pz,
                 const float *lo = LO3, const float *hi = HI3)
{
	Spec s{};
	s.name = name; s.kind = kind; s.C = C; s.A = A; s.S = S; s.grid = grid;
	s.points[0] = px; s.points[1] = py; s.points[2] = pz;
	for (int k = 0; k < 3; k++) { s.lo[k] = lo[k]; s.hi[k] = hi[k]; }
	return s;
}

static void grid_transform(Grid grid, const float *lo, const float *hi, float *m)
{
	for (int i = 0; i < 16; i++) m[i] = 0.f;
	m[15] = 1.f;
	switch (grid) {
	case Volume: case Tilted:
		m[0] = hi[0] - lo[0]; m[5] = hi[1] - lo[1]; m[10] = hi[2] - lo[2];
		m[12] = lo[0]; m[13] = lo[1]; m[14] = lo[2];
		break;
	case PlaneXZ: m[0] = hi[0] - lo[0]; m[6] = hi[2] - lo[2]; m[9] = 1.f;  m[12] = lo[0]; m[14] = lo[2]; break;
	case PlaneYZ: m[1] = hi[1] - lo[1]; m[6] = hi[2] - lo[2]; m[8] = -1.f; m[13] = lo[1]; m[14] = lo[2]; break;
	}
	if (grid == Tilted) {
		const float c = 0.98480775f, s = 0.17364818f;
		float r[16] = {c, 0, -s, 0,  0, 1, 0, 0,  s, 0, c, 0,  0, 0, 0, 1}, t[16];
		m4_mul(r, m, t);
		std::memcpy(m, t, sizeof t);
	}
}

static void make_block(const Spec &s, ParameterBlock &pb)
{
	pb = ParameterBlock{};
	BeamformerParameters &bp = pb.parameters;
	grid_transform(s.grid, s.lo, s.hi, bp.das_voxel_transform);
	for (int i = 0; i < 16; i++) bp.xdc_transform[i] = i % 5 == 0 ? 1.f : 0.f;
	const bool rca = s.kind == BeamformerAcquisitionKind_RCA_TPW || s.kind == BeamformerAcquisitionKind_RCA_VLS || s.kind == BeamformerAcquisitionKind_Flash;
	const bool hercules = s.kind == BeamformerAcquisitionKind_HERCULES || s.kind == BeamformerAcquisitionKind_UHERCULES || s.kind == BeamformerAcquisitionKind_HERO_PA;
	const float half = (float)(s.C - 1) / 2.f * s.pitch;
	const bool rows = (s.orientation & 0xF) == 1 || ((s.orientation >> 4) & 0xF) == 1;
	bp.xdc_transform[12] = half;
	bp.xdc_transform[13] = hercules ? (float)(s.A - 1) / 2.f * s.pitch : rca ? (rows ? half : 0.f) : half;
	bp.xdc_element_pitch[0] = bp.xdc_element_pitch[1] = s.pitch;
	bp.raw_data_dimensions[0] = s.S * s.A; bp.raw_data_dimensions[1] = s.C;
	bp.sample_count = s.S; bp.channel_count = s.C; bp.acquisition_count = s.A;
	bp.acquisition_kind = (BeamformerAcquisitionKind)s.kind;
	bp.sampling_frequency = s.fs; bp.demodulation_frequency = s.fs / 2.f; bp.speed_of_sound = 1540.f; bp.f_number = s.f_number;
	bp.interpolation_mode = (BeamformerInterpolationMode)s.interpolation;
	bp.coherency_weighting = s.cw; bp.decimation_rate = 1;
	for (int k = 0; k < 3; k++) bp.output_points[k] = (int32_t)s.points[k];
	bp.output_points[3] = 1;
	bp.single_focus = bp.single_orientation = s.A == 1 || !rca;
	bp.transmit_receive_orientation = s.orientation;
	static const float depths[8] = {-12e-3f, 30e-3f, -20e-3f, 45e-3f, 25e-3f, -15e-3f, 60e-3f, -30e-3f};
	for (uint32_t a = 0; a < s.A; a++) {
		pb.focal_vectors[a][0] = s.A > 1 ? -s.angle_span + 2.f * s.angle_span * (float)a / (float)(s.A - 1) : 0.f;
		pb.focal_vectors[a][1] = s.focused ? depths[a % 8] : __builtin_inff();
		pb.transmit_receive_orientations[a] = (uint8_t)(s.mixed_orientations && (a & 1) ? ((s.orientation & 0xF) << 4 | s.orientation >> 4) : s.orientation);
	}
	bp.focal_vector[0] = rca ? pb.focal_vectors[0][0] : 0.f; bp.focal_vector[1] = pb.focal_vectors[0][1];
	for (uint32_t c = 0; c < s.C; c++) pb.channel_mapping[c] = (int16_t)c;
	if (s.sparse) for (uint32_t a = 0; a + 1 < s.A; a++) pb.sparse_elements[a] = (int16_t)((a * 2 + 1) % s.C);
	bp.readi_group_count = s.readi_groups; bp.readi_group = s.readi_group;
	pb.shard_z_first = s.shard_first; pb.shard_z_count = s.shard_count;
	pb.data_kind = s.stages == DemodulateDas ? BeamformerDataKind_Int16 : s.iq ? BeamformerDataKind_Float32Complex : BeamformerDataKind_Float32;
	if (s.stages == DemodulateDas) {
		pb.shader_count = 2; pb.shaders[0] = BeamformerShaderKind_Demodulate; pb.shaders[1] = BeamformerShaderKind_DAS;
		BeamformerFilterParameters &f = pb.filters[0];
		f.kind = BeamformerFilterKind_Kaiser; f.sampling_frequency = s.fs / 2.f; f.complex = 0;
		f.kaiser.cutoff_frequency = s.fs / 8.f; f.kaiser.beta = 5.65f; f.kaiser.length = 36;
	} else if (s.stages == DasOnly) {
		pb.shader_count = 1; pb.shaders[0] = BeamformerShaderKind_DAS;
	}
}

static std::vector<Spec> lattice()
{
	const int TPW = BeamformerAcquisitionKind_RCA_TPW, VLS = BeamformerAcquisitionKind_RCA_VLS, Flash = BeamformerAcquisitionKind_Flash;
	const int FORCES = BeamformerAcquisitionKind_FORCES, UFORCES = BeamformerAcquisitionKind_UFORCES;
	const int HERC = BeamformerAcquisitionKind_HERCULES, UHERC = BeamformerAcquisitionKind_UHERCULES, HERO = BeamformerAcquisitionKind_HERO_PA;
	const int RACES = BeamformerAcquisitionKind_RACES;         /* das.glsl has no branch for it: the voxel stays zero */
	std::vector<Spec> v;
	Spec s;
	/* RCA on the general kernel: planes (depth on voxel y), few transmits */
	static const float lo1[3] = {-9.6e-3f, 0, 5e-3f}, hi1[3] = {9.6e-3f, 0, 25e-3f};
	s = spec("flash_plane", Flash, 64, 1, 1024, PlaneXZ, 256, 256, 1, lo1, hi1); s.orientation = 0x22; s.f_number = 1.f; v.push_back(s);
	s = spec("tpw_plane_small_real_cubic", TPW, 16, 2, 512, PlaneXZ, 48, 40, 1); s.orientation = 0x22; s.iq = false; s.interpolation = 2; s.fs = 25e6f; v.push_back(s);
	s = spec("flash_none_tx", Flash, 16, 1, 512, PlaneXZ, 16, 16, 1); s.orientation = 0x02; v.push_back(s);
	s = spec("tpw_plane_yz", TPW, 16, 2, 512, PlaneYZ, 40, 24, 1); s.orientation = 0x11; v.push_back(s);
	s = spec("tpw_demodulated", TPW, 32, 2, 1024, PlaneXZ, 64, 64, 1); s.orientation = 0x22; s.stages = DemodulateDas; s.fs = 25e6f; v.push_back(s);
	s = spec("tpw_mixed_orientations", TPW, 16, 4, 512, Volume, 12, 10, 14); s.mixed_orientations = true; s.cw = true; v.push_back(s);
	s = spec("tpw_tilted_big", TPW, 16, 2, 1024, Tilted, 64, 64, 64); v.push_back(s);
	/* RCA volumes whose delays separate: gather, staged in its forms, cut by the row-end rule */
	s = spec("tpw_volume_2tx", TPW, 32, 2, 1024, Volume, 64, 64, 64); v.push_back(s);
	s = spec("tpw_gather_5tx", TPW, 32, 5, 1024, Volume, 40, 36, 3); s.cw = true; v.push_back(s);
	s = spec("tpw_staged_short_rows", TPW, 32, 13, 256, Volume, 40, 36, 3); s.cw = true; v.push_back(s);
	s = spec("tpw_staged_short_rows_shard", TPW, 32, 13, 256, Volume, 40, 36, 3); s.cw = true; s.shard_first = 1; s.shard_count = 2; v.push_back(s);
	s = spec("tpw_staged_6tx", TPW, 32, 6, 1024, Volume, 40, 36, 3); v.push_back(s);
	s = spec("tpw_staged_fine", TPW, 32, 13, 1024, Volume, 150, 36, 3); s.cw = true; v.push_back(s);
	s = spec("tpw_staged_real", TPW, 32, 9, 1024, Volume, 40, 36, 3); s.iq = false; s.fs = 25e6f; v.push_back(s);
	s = spec("tpw_staged_cubic", TPW, 32, 9, 1024, Volume, 40, 36, 3); s.interpolation = 2; s.cw = true; v.push_back(s);
	s = spec("tpw_staged_rows_21", TPW, 48, 7, 1024, Volume, 45, 70, 2); s.orientation = 0x21; s.cw = true; v.push_back(s);
	s = spec("vls_staged", VLS, 32, 8, 1024, Volume, 40, 36, 3); s.focused = true; s.angle_span = 8.f; v.push_back(s);
	static const float lo_wide[3] = {-14e-3f, -14e-3f, 6e-3f}, hi_wide[3] = {14e-3f, 14e-3f, 9e-3f};
	s = spec("tpw_too_wide", TPW, 16, 6, 1024, Volume, 24, 24, 2, lo_wide, hi_wide); s.f_number = 0.2f; s.angle_span = 10.f; v.push_back(s);
	s = spec("tpw_sep_cubic_5tx", TPW, 32, 5, 512, Volume, 21, 37, 5); s.interpolation = 2; v.push_back(s);
	s = spec("tpw_sep_nearest_real", TPW, 16, 3, 512, Volume, 19, 18, 3); s.interpolation = 0; s.iq = false; s.fs = 25e6f; v.push_back(s);
	s = spec("tpw_narrow_nearest", TPW, 16, 3, 512, Volume, 24, 1, 40); s.interpolation = 0; s.orientation = 0x22; v.push_back(s);
	s = spec("tpw_tilted_8tx", TPW, 32, 8, 1024, Tilted, 40, 36, 3); v.push_back(s);
	/* the block-staged factored kernel: fine planes, a coarse one, a small one, a thin volume */
	static const float lo_t[3] = {-2e-3f, 0, 6e-3f}, hi_t[3] = {2e-3f, 0, 9.3e-3f}, hi_t64[3] = {2e-3f, 0, 13e-3f};
	s = spec("tile_tpw", TPW, 24, 9, 384, PlaneXZ, 160, 48, 1, lo_t, hi_t); s.interpolation = 2; s.orientation = 0x22; s.f_number = 1.f; s.pitch = 0.2e-3f; s.angle_span = 10.f; v.push_back(s);
	s = spec("tile_tpw_w64", TPW, 24, 9, 384, PlaneXZ, 160, 48, 1, lo_t, hi_t64); s.interpolation = 2; s.orientation = 0x22; s.f_number = 1.f; s.pitch = 0.2e-3f; s.angle_span = 10.f; v.push_back(s);
	static const float lo_c[3] = {-19e-3f, 0, 5e-3f}, hi_c[3] = {19e-3f, 0, 40e-3f};
	s = spec("tile_coarse", TPW, 64, 5, 1024, PlaneXZ, 512, 512, 1, lo_c, hi_c); s.interpolation = 2; s.orientation = 0x22; s.f_number = 0.3f; s.pitch = 0.2e-3f; v.push_back(s);
	static const float lo_s[3] = {-1.2e-3f, 0, 9.5e-3f}, hi_s[3] = {1.2e-3f, 0, 12.2e-3f};
	s = spec("tile_small_short_rows", TPW, 18, 7, 192, PlaneXZ, 96, 40, 1, lo_s, hi_s); s.interpolation = 2; s.orientation = 0x22; s.cw = true; s.f_number = 0.8f; s.pitch = 0.2e-3f; s.angle_span = 8.f; v.push_back(s);
	static const float lo_f[3] = {-3.2e-3f, 0, 6e-3f}, hi_f[3] = {3.2e-3f, 0, 12e-3f};
	s = spec("tile_big_short_rows", TPW, 24, 9, 176, PlaneXZ, 512, 512, 1, lo_f, hi_f); s.interpolation = 2; s.orientation = 0x22; s.f_number = 1.f; s.pitch = 0.2e-3f; s.angle_span = 10.f; v.push_back(s);
	static const float lo_v[3] = {-1.4e-3f, -0.3e-3f, 7e-3f}, hi_v[3] = {1.4e-3f, 0.3e-3f, 7.5e-3f};
	s = spec("tile_thin_volume", TPW, 16, 8, 384, Volume, 96, 6, 6, lo_v, hi_v); s.interpolation = 2; s.orientation = 0x22; s.cw = true; s.f_number = 1.f; s.pitch = 0.2e-3f; s.angle_span = 8.f; v.push_back(s);
	/* FORCES, UFORCES, READI */
	s = spec("forces", FORCES, 16, 16, 512, Volume, 20, 1, 20); v.push_back(s);
	s = spec("forces_shard", FORCES, 16, 16, 512, Volume, 20, 1, 20); s.shard_first = 5; s.shard_count = 8; v.push_back(s);
	s = spec("forces_2tx_real", FORCES, 16, 2, 512, Volume, 12, 12, 1); s.iq = false; s.fs = 25e6f; v.push_back(s);
	static const float lo_tf[3] = {-1.5e-3f, 0, 8e-3f}, hi_tf[3] = {1.5e-3f, 0, 10e-3f};
	s = spec("tile_forces", FORCES, 16, 16, 256, Volume, 96, 1, 40, lo_tf, hi_tf); s.interpolation = 2; s.f_number = 0.9f; s.pitch = 0.2e-3f; v.push_back(s);
	s = spec("tile_uforces_sparse", UFORCES, 16, 8, 256, Volume, 64, 1, 48, lo_tf, hi_tf); s.interpolation = 2; s.cw = true; s.sparse = true; s.f_number = 0.9f; s.pitch = 0.2e-3f; v.push_back(s);
	s = spec("uforces_sparse_nearest", UFORCES, 16, 8, 512, Volume, 16, 1, 16); s.interpolation = 0; s.sparse = true; s.iq = false; s.fs = 25e6f; v.push_back(s);
	s = spec("readi_4", FORCES, 16, 4, 512, Volume, 16, 1, 16); s.readi_groups = 4; s.readi_group = 2; v.push_back(s);
	s = spec("readi_8_cubic", UFORCES, 16, 2, 512, Volume, 40, 1, 40); s.readi_groups = 8; s.readi_group = 7; s.interpolation = 2; v.push_back(s);
	s = spec("readi_16_real", FORCES, 16, 4, 512, Volume, 64, 1, 64); s.readi_groups = 16; s.iq = false; s.fs = 25e6f; v.push_back(s);
	s = spec("readi_2_shard", FORCES, 16, 16, 512, Volume, 20, 1, 20); s.readi_groups = 2; s.readi_group = 1; s.shard_first = 3; s.shard_count = 9; v.push_back(s);
	s = spec("readi_4_no_das", FORCES, 16, 4, 512, Volume, 16, 1, 16); s.readi_groups = 4; s.stages = NoDas; v.push_back(s);
	/* HERCULES family */
	s = spec("hercules_wide_cw", HERC, 7, 16, 512, Volume, 64, 6, 3); s.cw = true; s.f_number = 0.7f; v.push_back(s);
	s = spec("hercules_narrow_real", HERC, 16, 8, 512, Volume, 10, 12, 14); s.iq = false; s.fs = 25e6f; s.f_number = 1.f; v.push_back(s);
	s = spec("uhercules_sparse_cubic", UHERC, 16, 8, 512, Volume, 48, 4, 2); s.sparse = true; s.interpolation = 2; v.push_back(s);
	s = spec("hercules_plane_xz_cubic", HERC, 7, 16, 512, PlaneXZ, 64, 48, 1); s.interpolation = 2; s.cw = true; s.f_number = 0.7f; v.push_back(s);
	s = spec("hercules_plane_yz", HERC, 7, 16, 512, PlaneYZ, 64, 40, 1); s.f_number = 0.7f; v.push_back(s);
	s = spec("hero_pa_nearest", HERO, 16, 8, 512, Volume, 32, 16, 2); s.interpolation = 0; v.push_back(s);
	s = spec("hercules_big", HERC, 16, 16, 1024, Volume, 128, 32, 64); v.push_back(s);
	s = spec("hercules_tilted", HERC, 16, 8, 512, Tilted, 64, 8, 4); v.push_back(s);
	/* what the shader leaves at zero; no DAS stage */
	s = spec("races_zero", RACES, 16, 4, 512, Volume, 20, 20, 2); v.push_back(s);
	s = spec("tpw_bad_interpolation", TPW, 16, 4, 512, PlaneXZ, 20, 20, 1); s.interpolation = 3; v.push_back(s);
	s = spec("flash_no_das", Flash, 16, 1, 512, PlaneXZ, 32, 32, 1); s.stages = NoDas; v.push_back(s);

	/* seeded picks from kinds x interpolation x data x transmit counts (both sides of kStagedMinTransmits and of the factored kernel's 3) x grids */
	static const struct { Grid grid; uint32_t p[3]; } grids[] = {
		{Volume, {40, 36, 3}}, {Volume, {20, 1, 24}}, {Volume, {70, 45, 2}}, {PlaneXZ, {96, 64, 1}}, {PlaneYZ, {33, 47, 1}}, {Tilted, {36, 40, 5}},
		{Volume, {128, 128, 20}}, {PlaneXZ, {24, 300, 1}},
	};
	static const int kinds[] = {TPW, VLS, Flash, FORCES, UFORCES, HERC, UHERC, HERO, RACES};
	static const uint32_t transmits[] = {2, 3, 5, 6, 7, 16};
	static char names[12][16];
	static const uint32_t channels[] = {16, 24, 64}, samples[] = {256, 1024}, orientations[] = {0x12, 0x21, 0x22, 0x11};
	static const float f_numbers[] = {0.5f, 1.f, 1.5f};
	uint64_t state = 0x9E3779B97F4A7C15ull;
	auto rng = [&]() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; };
	for (int i = 0; i < 12; i++) {
		std::snprintf(names[i], sizeof names[i], "seeded_%02d", i);
		const auto &g = grids[rng() % 8];
		s = spec(names[i], kinds[rng() % 9], channels[rng() % 3], transmits[rng() % 6], samples[rng() % 2], g.grid, g.p[0], g.p[1], g.p[2]);
		s.interpolation = (int)(rng() % 3); s.iq = rng() % 2; if (!s.iq) s.fs = 25e6f;
		s.cw = rng() % 2; s.orientation = orientations[rng() % 4];
		s.sparse = s.kind == UFORCES || s.kind == UHERC;
		s.f_number = f_numbers[rng() % 3];
		v.push_back(s);
	}
	return v;
}

/* ---------------------------------------------------------------- a run */

static const uint32_t kModes[] = {0, 1, 2, 3, 4, 6, 0x10, 0x100, 0x200, 0x400, 0x800, 0x1000, 0x4000, 0x8000};

static bool g_full = false;

static bool run(const Spec &s, uint32_t mode, const char *hook, const char *value)
{
	ParameterBlock pb;
	make_block(s, pb);
	Plan plan;
	std::string error;
	if (!build_plan(pb, plan, error, false)) { std::fprintf(stderr, "%s: the planner refuses the block: %s\n", s.name, error.c_str()); return false; }
	if (hook && !set_hook(hook, value)) return false;
	T.clear();
	const std::vector<BfTransmit> tx = build_transmit_table(pb);
	uint32_t zfirst = 0, zcount = plan.output_points[2];
	if (pb.shard_z_count) { zfirst = pb.shard_z_first; zcount = pb.shard_z_count; }

	std::vector<DasDecision> parts;
	decide_das_parts(pb, plan, tx, zfirst, zcount, mode, parts);
	dump("parts", parts);
	std::string paths;
	for (const DasDecision &d : parts) { if (!paths.empty()) paths += ','; paths += (char)('0' + d.path); }

	for (uint32_t n : {kBurstMinFrames - 1, kBurstMinFrames}) {
		BurstDecision b;
		decide_burst(pb, plan, tx, parts, zfirst, zcount, mode, n, b, false);
		put("frames", n); dump("burst", b);
	}
	for (uint32_t n : {kReadiSweepMinFrames - 1, kReadiSweepMinFrames}) {
		BurstDecision b;
		decide_burst(pb, plan, tx, parts, zfirst, zcount, mode, n, b, true);
		put("frames", n); dump("sweep", b);
	}

	/* views: the block's own grid, a plane of one 256-voxel tile, a volume; and the one-tile plane alone */
	ViewGrid views[3];
	std::memcpy(views[0].transform, pb.parameters.das_voxel_transform, sizeof views[0].transform);
	for (int k = 0; k < 3; k++) views[0].points[k] = plan.output_points[k];
	static const float lo_p[3] = {-2e-3f, 0, 8e-3f}, hi_p[3] = {2e-3f, 0, 12e-3f};
	grid_transform(PlaneXZ, lo_p, hi_p, views[1].transform); views[1].points[0] = 16; views[1].points[1] = 16; views[1].points[2] = 1;
	grid_transform(Volume, LO3, HI3, views[2].transform);    views[2].points[0] = 40; views[2].points[1] = 36; views[2].points[2] = 3;
	for (int set = 0; set < 2; set++) {
		const ViewGrid *list = set ? views + 1 : views;
		const uint32_t count = set ? 1 : 3;
		ViewsDecision vd;
		decide_views(pb, plan, tx, list, count, mode, vd);
		dump("views", vd, count, true);
		for (uint32_t n : {kBurstViewsMinFrames - 1, kBurstViewsMinFrames}) {
			BurstViewsDecision bv;
			decide_burst_views(pb, plan, tx, list, count, mode, n, bv);
			put("frames", n); dump("burst_views", bv, count);
		}
	}

	/* variants: below and at kVariantsMinVariants; then every second one known from the call before */
	DasVariant variants[kVariantsMinVariants];
	for (uint32_t k = 0; k < kVariantsMinVariants; k++) {
		variants[k].speed_of_sound = pb.parameters.speed_of_sound + 10.f * (float)k - 30.f;
		variants[k].time_offset    = pb.parameters.time_offset + 1e-7f * (float)(k % 3);
		variants[k].f_number       = pb.parameters.f_number * (1.f + 0.125f * (float)(k % 4));
	}
	VariantsDecision below, at, again;
	decide_variants(pb, plan, tx, variants, kVariantsMinVariants - 1, mode, below);
	dump("variants_below", below);
	decide_variants(pb, plan, tx, variants, kVariantsMinVariants, mode, at);
	dump("variants_at", at);
	const std::vector<DasDecision> *known[kVariantsMinVariants];
	for (uint32_t k = 0; k < kVariantsMinVariants; k++) known[k] = (k & 1) || at.parts[k].empty() ? nullptr : &at.parts[k];
	decide_variants(pb, plan, tx, variants, kVariantsMinVariants, mode, again, known);
	dump("variants_known", again);

	if (pb.parameters.readi_group_count > 1) {
		ParameterBlock derived;
		Plan derived_plan;
		derive_readi_image(pb, plan, derived, derived_plan);
		std::vector<DasDecision> image_parts;
		if (derived_plan.das_index >= 0 && zcount) decide_das_parts(derived, derived_plan, build_transmit_table(derived), zfirst, zcount, mode, image_parts);
		dump("image_parts", image_parts);
		ReadiImageDecision image;
		decide_readi_image(derived_plan, image_parts, pb.parameters.readi_group_count, pb.parameters.readi_group_count, image);
		dump("image", image);
	}
	if (hook) set_hook(hook, nullptr);

	uint64_t h = 0xcbf29ce484222325ull;
	for (unsigned char c : T) { h ^= c; h *= 0x100000001b3ull; }
	char id[96];
	if (hook) std::snprintf(id, sizeof id, "%s/%x/%s=%s", s.name, mode, hook, value);
	else      std::snprintf(id, sizeof id, "%s/%x", s.name, mode);
	if (g_full) std::printf("%s %s\n", id, T.c_str());
	else        std::printf("%s %s %zu %016llx\n", id, paths.c_str(), parts.size(), (unsigned long long)h);
	return true;
}

int main(int argc, char **argv)
{
	bool coverage = false;
	for (int i = 1; i < argc; i++) {
		if (!std::strcmp(argv[i], "--full")) g_full = true;
		else if (!std::strcmp(argv[i], "--coverage")) coverage = true;
		else { std::fprintf(stderr, "usage: select_digest [--full] [--coverage]\n"); return 1; }
	}
	const std::vector<Spec> blocks = lattice();
	for (const Spec &s : blocks)
		for (uint32_t mode : kModes) if (!run(s, mode, nullptr, nullptr)) return 1;
	/* the hooks that change a decision, on the blocks the staged kernels take */
	static const char *const hooked[] = {"tpw_staged_6tx", "tpw_staged_fine", "tpw_staged_short_rows", "tpw_staged_real", "tpw_staged_cubic", "tpw_gather_5tx"};
	static const char *const hooks_set[][2] = {{"STAGED_SHAPE", "5,5,5"}, {"STAGED_SHAPE", "6,4,6"}, {"STAGED_SHAPE", "4,5,5"}, {"STAGED_SHAPE", "5,4,6"},
	                                           {"STAGED_NOUNIFORM", "1"}, {"STAGED_TABLE_CAP", "0"}};
	for (const Spec &s : blocks)
		for (const char *name : hooked) if (!std::strcmp(s.name, name))
			for (const auto &h : hooks_set)
				for (uint32_t mode : {0u, 3u}) if (!run(s, mode, h[0], h[1])) return 1;

	static const char *const required[] = {
		"path 0", "path 1", "path 2", "path 3", "path 4", "path 5", "path 7",
		"staged: global tables", "staged: LDS tables", "staged: the table cap sends it to the LDS-table shape",
		"a frame cut into parts by the row-end rule", "channel split on", "channel split off",
		"tile: taken", "tile: estimated away", "tile: forbidden",
		"burst: taken", "burst: the sweep kernel taken", "burst declined: no DAS stage runs", "burst declined: acquisition kind or interpolation",
		"burst declined: das path flag 0x400", "burst declined: the burst kernel exists for", "burst declined: the row-end rule cuts",
		"burst declined: single frames run the", "burst declined: fewer than",
		"views: all taken", "views: some taken", "views: none taken", "burst views: rung 1", "burst views: rung 2", "burst views: rung 3",
		"variants: taken by count", "variants: taken by tiles", "variants: declined below both thresholds",
		"READI image: a DAS stage", "READI image: no DAS stage",
	};
	/* reported, not required: no block was found that reaches it (the LDS-table shape of a frame the global-table forms take fits the LDS
	 * wherever the element bound (A4 << window_shift) <= 4096 lets the form be planned at all) */
	static const char *const reported[] = {"staged: the table cap sends it to the gather kernel"};
	bool ok = true;
	for (const char *item : required) {
		const unsigned long n = reached.count(item) ? reached[item] : 0;
		if (coverage) std::fprintf(g_full ? stderr : stdout, "# %-60s %lu\n", item, n);
		if (!n) { std::fprintf(stderr, "the lattice does not reach: %s\n", item); ok = false; }
	}
	if (coverage) for (const char *item : reported) std::fprintf(g_full ? stderr : stdout, "# %-60s %lu (not required)\n", item, reached.count(item) ? reached[item] : 0);
	return ok ? 0 : 2;
}
