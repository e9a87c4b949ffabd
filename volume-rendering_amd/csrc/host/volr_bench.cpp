// volr_bench — headless command-line driver over the host mirror: the reference's start-up sequence
// (VolR.cpp:352-442) without GLUT/GLUI, its benchmark loop and configuration matrix (VolR.cpp:225-321), its profiler
// summary table (VolR.cpp:200-223) and, for eyeballing, a PPM writer for single frames.  There is no interactive mode.
//
//   volr_bench [-h] [-f <file.pvm|.raw>] [-raw <w> <h> <d> [<bytes>]] [-synthetic <n>] [-dir <datasets>] [-r <id>]
//              [-s <width> <height>] [-d <device>] [-devices <a,b,..>] [-b|-bg] [-pose <ax> <ay> <az> <dist>] [-persp] [-mip] [-iso <level> [-refine <n>]]
//              [-clip-box <x0> <y0> <z0> <x1> <y1> <z1>] [-clip-plane <nx> <ny> <nz> <d>] [-shadow <S> [-shadow-strength <s>] [-shadow-step <t>]]
//              [-phong <ka> <kd> <ks> <n>] [-preint] [-hybrid <level> [-refine <n>]]
//              [-section <nx> <ny> <nz> <d> [-section-half <h>] [-section-mode max|min|mean] [-section-window <lo> <hi>] [-section-in-volume]]
//              [-depth <opacity> [-depth-mode first|peak|mean] [-pick <x> <y>]] [-labels <file.raw> | -labels-octants] [-label <id> <r> <g> <b> <mix> <opacity>]...
//              [-o <frame.ppm>]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "ModelBase.h"
#include "frame_stats.h"
#include "RaycasterBase.h"
#include "camera.h"

using namespace volr;

namespace {

const float MAX_BENCH_SAMPLE = 7500;         // VolR.cpp:26: a renderer is dropped from a configuration after a 7.5 s frame

int config = 0, device = 0, renderer_id = 1;
std::vector<std::string> row_names = { "Interactive" };     // profiler row labels: row 0 is the interactive / single-frame row
std::vector<int> device_list;       // -devices a,b,c: one frame split over several GPUs (vr_hip_multi_*)
std::string dataset_dir = ".";
unsigned synthetic_n = 0;
std::vector<unsigned char> synthetic_voxels;
std::vector<uchar4> frame;
HipRenderer *renderers[PROFILER_RENDERERS] = { nullptr, nullptr };

void print_usage() {
	printf("volr_bench - headless MI355X volume raycaster driver (benchmark matrix of VolR -b)\n\n"
	       "  -h : this help\n  -f <file> : volume data, .pvm or .raw (with -raw <w> <h> <d> [<bytes per voxel>])\n"
	       "  -synthetic <n> : n^3 synthetic shell volume (stands in for missing datasets in benchmark mode)\n"
	       "  -dir <path> : directory searched for <Name>.pvm in benchmark mode (default .)\n"
	       "  -r <id> : renderer, 0 = HIP nearest (CPURenderer semantics), 1 = HIP trilinear (GPURenderer4 semantics)\n"
	       "  -s <width> <height> : viewport, 128..2048 like the reference\n  -d <device> : GPU index\n"
	       "  -devices <a,b,...> : split every frame over these GPUs (interleaved bands gathered on the first one over xGMI)\n"
	       "  -mip : maximum-intensity projection instead of the composite (single device)\n"
	       "  -iso <level> [-refine <n>] : shaded isosurface at <level> (raw voxel units), n bisection steps (default 4, 0..16), from the\n"
	       "         trilinear renderer (-r 1; renderer 0 keeps compositing in benchmark mode); single device, excludes -mip\n"
	       "  -clip-box <x0> <y0> <z0> <x1> <y1> <z1> : crop every frame to this box (model space: the volume is [-1,1]^3)\n"
	       "  -clip-plane <nx> <ny> <nz> <d> : keep the half-space nx*x + ny*y + nz*z + d >= 0; both work with the composite, -mip and -iso\n"
	       "  -shadow <S> [-shadow-strength <s>] [-shadow-step <t>] : light-source shadows for the composite of the trilinear renderer (-r 1): a light\n"
	       "         grid of S^3 nodes (2..256) marched towards the view's light; strength 0..1 (default 1), step in model units (default: the ray step)\n"
	       "  -phong <ka> <kd> <ks> <n> : gradient lighting for the composite of the trilinear renderer (-r 1): ambient, diffuse and specular\n"
	       "         coefficients 0..1 and shininess_log2 0..10 (the highlight is raised to the power 2^n); composes with -shadow and the clip\n"
	       "  -preint : pre-integrated (slab) classification for the composite of the trilinear renderer (-r 1): a sample takes the mean of the\n"
	       "         transfer function between the previous sample's value and its own; composes with the clip, -shadow and -phong\n"
	       "  -hybrid <level> [-refine <n>] : the isosurface at <level> seen through the translucent volume in front of it (the isosurface frame, then\n"
	       "         the composite stopped at its depth and blended over it), from the trilinear renderer (-r 1); single device; works alone and with\n"
	       "         the clip, -shadow, -phong and -preint, which the composite pass sees; excludes -mip, -iso and -devices\n"
	       "  -section <nx> <ny> <nz> <d> [-section-half <h>] [-section-mode max|min|mean] [-section-window <lo> <hi>] [-section-in-volume] : the section\n"
	       "         nx*x + ny*y + nz*z + d = 0 through the interpolated field (model space); with -section-half h > 0 the maximum (default), minimum\n"
	       "         or mean over the slab of that half width; -section-window: opaque grey between lo and hi (raw voxel units) instead of the transfer\n"
	       "         function; -section-in-volume: the section seen through the translucent volume in front of it (the composite pass sees the clip,\n"
	       "         -shadow, -phong and -preint); from the trilinear renderer (-r 1); single device; excludes -mip, -iso, -hybrid and -devices\n"
	       "  -labels <file.raw> | -labels-octants, -label <id> <r> <g> <b> <mix> <opacity> (repeatable) : the labelled composite frame: a second volume\n"
	       "         of one byte per voxel (a raw file of the volume's dims, x fastest, or the voxel's octant 0..7) names each voxel's segment, and the\n"
	       "         table entry of a label tints (mix), replaces (mix 1), fades (opacity) or hides (opacity 0) what the transfer function returns\n"
	       "         there; labels without an entry stay as they are; from the trilinear renderer (-r 1); single device; works with the clip, -shadow\n"
	       "         and -phong; excludes -mip, -iso, -hybrid, -section, -depth, -preint and -devices\n"
	       "  -depth <opacity> [-depth-mode first|peak|mean] [-pick <x> <y>] : the depth frame of the composite instead of its colours: where along\n"
	       "         its ray the thing a pixel shows lies — the first sample at which the accumulated alpha reaches <opacity> (default), the sample\n"
	       "         that contributes most, or the contribution-weighted mean; -o writes the depth of the hits as a normalised grey image (near =\n"
	       "         bright, no surface = black); -pick prints position, voxel index, value and alpha of pixel (x, y), y up; the clip and -preint\n"
	       "         apply; from the trilinear renderer (-r 1); single device, single frame; excludes -mip, -iso, -hybrid and -section\n"
	       "  -b | -bg : benchmark mode\n  -pose <ax> <ay> <az> <dist> [-persp] -o <frame.ppm> : render one frame to a PPM file\n");
}

// SURVEY §8(d) "shell": deterministic integer-only test volume (same generator as the GPU kernel and the oracle)
void make_shell(unsigned n, std::vector<unsigned char> *out) {
	out->resize((size_t) n * n * n);
	const long long N = n;
	for (long long z = 0; z < N; z++)
		for (long long y = 0; y < N; y++)
			for (long long x = 0; x < N; x++) {
				const unsigned long long idx = ((unsigned long long) z * N + y) * N + x;
				unsigned h = (unsigned) (idx ^ (idx >> 32)) + 1u * 0x9E3779B9u;
				h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
				const long long ax = 2 * x + 1 - N, ay = 2 * y + 1 - N, az = 2 * z + 1 - N;
				long long t = 1000 * (ax * ax + ay * ay + az * az) / (N * N) - 360;
				if (t < 0) t = -t;
				long long shell = 255 - t * 255 / 240;
				if (shell < 0) shell = 0;
				unsigned v = (unsigned) shell + (h & 15u);
				(*out)[idx] = (unsigned char) (v > 255u ? 255u : v);
			}
}

bool use_synthetic() {
	if (synthetic_n == 0) return false;
	if (synthetic_voxels.empty()) make_shell(synthetic_n, &synthetic_voxels);
	// ModelBase owns (and frees) its voxel buffer like the reference does (ModelBase.cpp:99-100): hand it a malloc'ed copy
	unsigned char *copy = (unsigned char *) malloc(synthetic_voxels.size());
	if (copy == NULL) return false;
	memcpy(copy, synthetic_voxels.data(), synthetic_voxels.size());
	if (ModelBase::volume.data != NULL) free(ModelBase::volume.data);
	ModelBase::volume.data = copy;
	ModelBase::volume.size = (unsigned) synthetic_voxels.size();
	ModelBase::volume.dims = make_ushort3((unsigned short) synthetic_n, (unsigned short) synthetic_n, (unsigned short) synthetic_n);
	return true;
}

// VolR.cpp:255-268 benchmark_load_file (+ every renderer's set_volume / set_transfer_fn)
int install_volume() {
	RaycasterBase::set_volume(ModelBase::volume);
	for (int i = 0; i < PROFILER_RENDERERS; i++) {
		if (renderers[i]->set_volume(RaycasterBase::raycaster.volume) != 0) return 1;
		renderers[i]->set_transfer_fn(RaycasterBase::raycaster);
	}
	return 0;
}

int benchmark_load_file(const char *name) {
	const std::string path = dataset_dir + "/" + name + ".pvm";
	if (ModelBase::load_model(path.c_str()) != 0) {
		printf("Error: File not found: %s\n", path.c_str());
		return 1;
	}
	return install_volume();
}

// VolR.cpp:98-113 draw_volume without the GL parts
void draw_volume() {
	if (frame.size() != (size_t) ViewBase::view.dims.x * ViewBase::view.dims.y) {
		frame.resize((size_t) ViewBase::view.dims.x * ViewBase::view.dims.y);
		for (int i = 0; i < PROFILER_RENDERERS; i++) renderers[i]->set_window_buffer(ViewBase::view);
	}
	RaycasterBase::set_view(ViewBase::view);
	Profiler::start(renderer_id);
	renderers[renderer_id]->render_volume(frame.data(), RaycasterBase::raycaster);
	Profiler::stop();
}

// VolR.cpp:225-253 benchmark_config_loop: every renderer x {orthogonal, perspective} x 4 poses at distance 2
void benchmark_config_loop() {
	static const float poses[4][3] = { { 0, 0, 0 }, { -45, -45, 0 }, { 90, 0, 0 }, { 180, 90, 0 } };
	Profiler::reset_config(config);
	for (renderer_id = 0; renderer_id < PROFILER_RENDERERS; renderer_id++) {
		ViewBase::view.perspective = false;
		bool timed_out = false;
		for (int p = 0; p < 2 && !timed_out; p++) {
			ViewBase::toggle_perspective(1);
			for (int i = 0; i < 4; i++) {
				ViewBase::set_camera_position(make_float3(poses[i][0], poses[i][1], poses[i][2]), 2);
				draw_volume();
				if (Profiler::time_ms > MAX_BENCH_SAMPLE) { timed_out = true; break; }
			}
			ViewBase::view.perspective = true;
		}
	}
	printf("%15s,", row_names[config].c_str());
	Profiler::print_avg(stdout, config);
	config++;
}

// ---- the reference's configuration matrix (VolR.cpp:270-321) as DATA: one row per configuration, one loop that runs them ----
struct BenchConfig {
	std::string name;            // row label of the profiler table (VolR.cpp:34-38)
	std::string dataset;         // "<name>.pvm" to load before the run; empty = keep the resident volume
	bool foot_study;             // part of the option / scale / ray-step studies the reference runs on "Foot"
	int esl;                     // empty-space leaping on (1) / off (0)
	float ray_threshold;         // early-ray-termination threshold
	float viewport_scale;        // 0 = the original viewport, else original * scale (ushort truncation, ViewBase.cpp:107-113)
	float ray_step_factor;       // 0 = the volume's default step, else default * factor
};

std::vector<BenchConfig> build_matrix() {
	std::vector<BenchConfig> m;
	for (const char *ds : { "Bucky", "Daisy", "VisMale", "Engine", "Foot", "Pig", "Porsche" })
		m.push_back({ ds, ds, false, 1, 0.95f, 0.0f, 0.0f });
	m.push_back({ "Foot: No optims", "", true, 0, 1.0f, 0.0f, 0.0f });
	m.push_back({ "F: ERT on", "", true, 0, 0.95f, 0.0f, 0.0f });
	m.push_back({ "F: ERT+ESL on", "", true, 1, 0.95f, 0.0f, 0.0f });
	// The reference steps both studies by repeated fp32 addition of 0.1 (0.9, 0.79999995, ... 0.29999992; 1.1 ... 1.7000002);
	// the accumulated values decide the truncated viewport sizes (2048 * 0.49999991 -> 1023), so they are reproduced here.
	float scale = 1.0f, factor = 1.0f;
	for (int tenth = 9; tenth >= 3; tenth--) {
		scale -= 0.1f;
		m.push_back({ "Scale 0." + std::to_string(tenth), "", true, 1, 0.95f, scale, 0.0f });
	}
	for (int tenth = 1; tenth <= 7; tenth++) {
		factor += 0.1f;
		m.push_back({ "Ray step *1." + std::to_string(tenth), "", true, 1, 0.95f, 0.0f, factor });
	}
	return m;
}

void benchmark() {
	printf("Entering benchmark loop...\n\n");
	const std::vector<BenchConfig> matrix = build_matrix();
	const ushort2 original_size = ViewBase::view.dims;
	bool foot_ready = false, foot_tried = false;
	config = 1;
	for (const BenchConfig &c : matrix) {
		if (c.foot_study && !foot_tried) {                   // the studies run on "Foot"; a synthetic volume may stand in
			foot_tried = true;
			foot_ready = benchmark_load_file("Foot") == 0;
			if (!foot_ready && use_synthetic()) {
				printf("(Foot.pvm not available: using the %u^3 synthetic shell for the remaining configurations)\n", synthetic_n);
				foot_ready = install_volume() == 0;
			}
		}
		if (c.foot_study && !foot_ready) break;
		row_names.push_back(c.name);
		printf("%s benchmark\n", c.name.c_str());
		if (!c.dataset.empty() && benchmark_load_file(c.dataset.c_str()) != 0) { config++; continue; }     // VolR.cpp:276-279: a missing file is skipped
		if ((RaycasterBase::raycaster.esl ? 1 : 0) != c.esl) RaycasterBase::toggle_esl();
		RaycasterBase::change_ray_threshold(c.ray_threshold, true);
		if (c.ray_step_factor > 0.0f) {
			RaycasterBase::reset_ray_step();
			RaycasterBase::change_ray_step(RaycasterBase::raycaster.ray_step * c.ray_step_factor, true);
		} else if (c.foot_study) {
			RaycasterBase::reset_ray_step();
		}
		if (c.viewport_scale > 0.0f) {
			ViewBase::set_viewport_dims(original_size, c.viewport_scale);
			printf("Resolution: %dx%d\n", ViewBase::view.dims.x, ViewBase::view.dims.y);
		} else if (ViewBase::view.dims.x != original_size.x || ViewBase::view.dims.y != original_size.y) {
			ViewBase::set_viewport_dims(original_size);
		}
		benchmark_config_loop();
	}
	RaycasterBase::reset_ray_step();
	ViewBase::set_viewport_dims(original_size);
	config--;
}

// VolR.cpp:200-223: the summary table — which statistics a row shows is a property of the row
void print_profiler() {
	printf("\nSummary profiler report:\n");
	for (int r = 0; r < PROFILER_RENDERERS; r++) printf(" Rend.%2i: %s\n", r, renderers[r]->get_name());
	printf("%15s,%8s,", "Configuration", "Value");
	for (int r = 0; r < PROFILER_RENDERERS; r++) printf(" Rend.%2i%s", r, r != PROFILER_RENDERERS - 1 ? "," : "");
	printf("\n");
	typedef void (*Stat)(FILE *, int);
	static const Stat interactive_stats[] = { Profiler::print_samples, Profiler::print_avg, Profiler::print_max };
	static const Stat config_stats[] = { Profiler::print_avg };
	for (int row = 0; row <= config && row < (int) row_names.size(); row++) {
		const Stat *stats = row == 0 ? interactive_stats : config_stats;
		const int count = row == 0 ? 3 : 1;
		for (int k = 0; k < count; k++) { printf("%15s,", row_names[row].c_str()); stats[k](stdout, row); }
	}
}

// premultiplied RGBA8, y-up (RaycasterBase.h:44-50) -> binary PPM over a black background, top row first
int write_ppm(const char *path) {
	FILE *f = fopen(path, "wb");
	if (f == NULL) return 1;
	const int w = ViewBase::view.dims.x, h = ViewBase::view.dims.y;
	fprintf(f, "P6\n%d %d\n255\n", w, h);
	for (int y = h - 1; y >= 0; y--)
		for (int x = 0; x < w; x++) {
			const uchar4 c = frame[(size_t) y * w + x];
			const unsigned char rgb[3] = { c.x, c.y, c.z };
			fwrite(rgb, 1, 3, f);
		}
	fclose(f);
	return 0;
}

// the depth of the hits as a grey image: near = 255, far = 1 over the range of the frame's surfaces, no surface = 0; top row first
int write_depth_ppm(const char *path, const std::vector<float> &depth) {
	FILE *f = fopen(path, "wb");
	if (f == NULL) return 1;
	const int w = ViewBase::view.dims.x, h = ViewBase::view.dims.y;
	float lo = 0.0f, hi = 0.0f;
	bool any = false;
	for (float d : depth)
		if (d >= 0.0f) { lo = any ? (d < lo ? d : lo) : d; hi = any ? (d > hi ? d : hi) : d; any = true; }
	fprintf(f, "P6\n%d %d\n255\n", w, h);
	for (int y = h - 1; y >= 0; y--)
		for (int x = 0; x < w; x++) {
			const float d = depth[(size_t) y * w + x];
			unsigned char g = 0;
			if (d >= 0.0f) {
				const float s = hi > lo ? (d - lo) / (hi - lo) : 0.0f;
				g = (unsigned char) (255.0f - s * 254.0f + 0.5f);
			}
			const unsigned char rgb[3] = { g, g, g };
			fwrite(rgb, 1, 3, f);
		}
	fclose(f);
	return 0;
}

// one depth frame of the trilinear renderer into `depth` (HipRenderer::render_depth), timed like draw_volume's frame
int draw_depth(const vr_depth &d, std::vector<float> &depth) {
	const size_t pixels = (size_t) ViewBase::view.dims.x * ViewBase::view.dims.y;
	if (frame.size() != pixels) {
		frame.resize(pixels);
		for (int i = 0; i < PROFILER_RENDERERS; i++) renderers[i]->set_window_buffer(ViewBase::view);
	}
	depth.assign(pixels, -1.0f);
	RaycasterBase::set_view(ViewBase::view);
	const vr_depth_out out = { depth.data(), nullptr, nullptr };
	Profiler::start(renderer_id);
	const int rc = renderers[1]->render_depth(RaycasterBase::raycaster, d, &out);
	Profiler::stop();
	return rc;
}

// ---- the command line ----
struct Options {
	std::string file_name, out_ppm, labels_file;
	bool loaded = false;                        // a volume is resident (main sets it after loading)
	bool benchmark_mode = false, persp = false, have_pose = false;
	float pose[4] = { 120, 0, 200, 3 };       // the reference's interactive start pose (VolR.cpp:436)
	bool mip = false, iso = false, hybrid = false, section_on = false, depth_on = false, labels_octants = false;       // the frame kinds (`kinds` below)
	float iso_level = 0.0f;                     // of -iso and -hybrid: the one given last
	int iso_refine = 4;
	bool section_in_volume = false, section_mode_given = false, section_window_given = false, depth_mode_given = false, pick_on = false;
	vr_section section = { { 0.0f, 0.0f, 0.0f, 0.0f }, 0.0f, VR_SECTION_POINT, { 0.0f, 0.0f } };
	vr_depth depth = { 0.5f, VR_DEPTH_FIRST };
	uint32_t pick_xy[2] = { 0u, 0u };
	uint32_t label_entries = 0;                 // entries of the table given so far: the highest -label id + 1
	std::vector<vr_label_entry> label_table = std::vector<vr_label_entry>(VR_LABEL_COUNT, vr_label_entry{ { 0.0f, 0.0f, 0.0f }, 0.0f, 1.0f });
	bool clip_box = false, clip_plane = false, phong = false, preint = false;       // state of every frame
	vr_clip clip = { { -1.0f, -1.0f, -1.0f }, { 1.0f, 1.0f, 1.0f }, { 0.0f, 0.0f, 0.0f, 0.0f } };
	vr_lighting lighting = { 0.25f, 0.65f, 0.4f, 4u };
	int shadow_dims = 0;
	float shadow_strength = 1.0f, shadow_step = 0.0f;
};

const char *const section_mode_names[] = { "point", "max", "min", "mean" }, *const depth_mode_names[] = { "first", "peak", "mean" };      // by vr_section_mode / vr_depth_mode

// Fills `o` (and the globals above) from the command line.  A refused option prints its message and is skipped, like the reference's
// parser; -h and two malformed values end the program: the exit status then, else -1.
int parse(int argc, char **argv, Options &o) {
	for (int i = 1; i < argc; i++) {
		const char *arg = argv[i];
		auto need = [&](int n) { if (i + n >= argc) { printf("%s error: Not enough parameters. Use -h to help.\n", arg); return false; } return true; };
		auto is = [&](const char *flag) { return strcmp(arg, flag) == 0; };
		auto number = [&]() { return (float) atof(argv[++i]); };
		auto mode = [&](const char *const *names, int first, int count) { const char *m = argv[++i]; for (int k = first; k < count; k++) if (strcmp(m, names[k]) == 0) return k; return -1; };
		if (is("-h")) { print_usage(); return EXIT_SUCCESS; }
		else if (is("-f")) { if (need(1)) o.file_name = argv[++i]; }
		else if (is("-raw")) {
			if (!need(3)) continue;
			const unsigned w = atoi(argv[i + 1]), h = atoi(argv[i + 2]), d = atoi(argv[i + 3]);
			i += 3;
			unsigned c = 1;
			if (i + 1 < argc && argv[i + 1][0] != '-') c = atoi(argv[++i]);
			ModelBase::set_raw_dims(w, h, d, c);
		}
		else if (is("-synthetic")) { if (need(1)) synthetic_n = atoi(argv[++i]); }
		else if (is("-dir")) { if (need(1)) dataset_dir = argv[++i]; }
		else if (is("-r")) {
			if (!need(1)) continue;
			const int r = atoi(argv[++i]);
			if (r < 0 || r >= PROFILER_RENDERERS) { printf("%s error: Wrong parameters. Use -h to help.\n", arg); continue; }
			renderer_id = r;
		}
		else if (is("-s")) {
			if (!need(2)) continue;
			const int w = atoi(argv[++i]), h = atoi(argv[++i]);
			if (w < 128 || h < 128 || w > 2048 || h > 2048) { printf("%s error: Wrong parameters. Use -h to help.\n", arg); continue; }   // VolR.cpp:392
			ViewBase::set_viewport_dims(make_ushort2((unsigned short) w, (unsigned short) h));
		}
		else if (is("-d")) { if (need(1)) device = atoi(argv[++i]); }
		else if (is("-devices")) {
			if (!need(1)) continue;
			for (const char *q = argv[++i]; *q; ) { device_list.push_back(atoi(q)); while (*q && *q != ',') q++; if (*q == ',') q++; }
		}
		else if (is("-bg") || is("-b")) o.benchmark_mode = true;
		else if (is("-persp")) o.persp = true;
		else if (is("-mip")) o.mip = true;
		else if (is("-iso")) { if (need(1)) { o.iso_level = number(); o.iso = true; } }
		else if (is("-hybrid")) { if (need(1)) { o.iso_level = number(); o.hybrid = true; } }
		else if (is("-section")) { if (need(4)) { for (int k = 0; k < 4; k++) o.section.plane[k] = number(); o.section_on = true; } }
		else if (is("-section-half")) { if (need(1)) o.section.half_width = number(); }
		else if (is("-section-mode")) {
			if (!need(1)) continue;
			const int m = mode(section_mode_names, 1, 4);           // "point" is what no -section-half gives, not a word of this option
			if (m < 0) { printf("%s error: Wrong parameters. Use -h to help.\n", arg); continue; }
			o.section.mode = (uint32_t) m; o.section_mode_given = true;
		}
		else if (is("-section-window")) { if (need(2)) { o.section.window[0] = number(); o.section.window[1] = number(); o.section_window_given = true; } }
		else if (is("-section-in-volume")) o.section_in_volume = true;
		else if (is("-depth")) { if (need(1)) { o.depth.opacity = number(); o.depth_on = true; } }
		else if (is("-depth-mode")) {
			if (!need(1)) continue;
			const int m = mode(depth_mode_names, 0, 3);
			if (m < 0) { printf("Error: -depth-mode takes first, peak or mean\n"); return EXIT_FAILURE; }
			o.depth.mode = (uint32_t) m; o.depth_mode_given = true;
		}
		else if (is("-pick")) { if (need(2)) { o.pick_xy[0] = (uint32_t) atoi(argv[++i]); o.pick_xy[1] = (uint32_t) atoi(argv[++i]); o.pick_on = true; } }
		else if (is("-labels")) { if (need(1)) o.labels_file = argv[++i]; }
		else if (is("-labels-octants")) o.labels_octants = true;
		else if (is("-label")) {
			if (!need(6)) continue;
			const int id = atoi(argv[++i]);
			vr_label_entry e;
			for (int k = 0; k < 3; k++) e.colour[k] = number();
			e.mix = number(); e.opacity = number();
			if (id < 0 || id >= VR_LABEL_COUNT) { printf("Error: -label takes an id in 0..255\n"); return EXIT_FAILURE; }
			o.label_table[(size_t) id] = e;
			if ((uint32_t) id + 1u > o.label_entries) o.label_entries = (uint32_t) id + 1u;
		}
		else if (is("-refine")) { if (need(1)) o.iso_refine = atoi(argv[++i]); }
		else if (is("-clip-box")) { if (need(6)) { for (int k = 0; k < 3; k++) o.clip.box_min[k] = number(); for (int k = 0; k < 3; k++) o.clip.box_max[k] = number(); o.clip_box = true; } }
		else if (is("-clip-plane")) { if (need(4)) { for (int k = 0; k < 4; k++) o.clip.plane[k] = number(); o.clip_plane = true; } }
		else if (is("-shadow")) { if (need(1)) o.shadow_dims = atoi(argv[++i]); }
		else if (is("-shadow-strength")) { if (need(1)) o.shadow_strength = number(); }
		else if (is("-shadow-step")) { if (need(1)) o.shadow_step = number(); }
		else if (is("-preint")) o.preint = true;
		else if (is("-phong")) {
			if (need(4)) { o.lighting.ambient = number(); o.lighting.diffuse = number(); o.lighting.specular = number(); o.lighting.shininess_log2 = (uint32_t) atoi(argv[++i]); o.phong = true; }
		}
		else if (is("-pose")) { if (need(4)) { for (int k = 0; k < 4; k++) o.pose[k] = number(); o.have_pose = true; } }
		else if (is("-o")) { if (need(1)) o.out_ppm = argv[++i]; }
		else printf("Warning: unknown argument: %s\n", arg);
	}
	return -1;
}

// "Error: <what the renderer says>" after a refused call
bool accepted(HipRenderer *renderer, int rc) { if (rc != 0) printf("Error: %s\n", renderer->last_error()); return rc == 0; }

// ---- the frame kinds.  apply: the kind's own last checks, its setter, its announcement; false = refused ----
bool apply_mip(Options &) { for (int i = 0; i < PROFILER_RENDERERS; i++) renderers[i]->set_mip(true); printf("Maximum-intensity projection\n"); return true; }
bool apply_iso(Options &o) { renderers[1]->set_iso(true, o.iso_level, (uint32_t) o.iso_refine); printf("Isosurface at level %g, %d bisection steps\n", o.iso_level, o.iso_refine); return true; }
bool apply_hybrid(Options &o) {
	renderers[1]->set_hybrid(true, o.iso_level, (uint32_t) o.iso_refine);
	printf("Hybrid: isosurface at level %g, %d bisection steps, behind the composite\n", o.iso_level, o.iso_refine);
	return true;
}
bool apply_section(Options &o) {
	vr_section &section = o.section;
	if (section.half_width > 0.0f && !o.section_mode_given) section.mode = VR_SECTION_MAX;      // a slab without a mode: the slab MIP
	renderers[1]->set_section(true, section, o.section_in_volume);
	printf("Section: plane %g x + %g y + %g z + %g = 0, half width %g, mode %s", section.plane[0], section.plane[1], section.plane[2], section.plane[3],
	       section.half_width, section_mode_names[section.mode & 3u]);
	if (section.window[0] != 0.0f || section.window[1] != 0.0f) printf(", grey window %g..%g", section.window[0], section.window[1]);
	printf(o.section_in_volume ? ", behind the composite\n" : "\n");
	return true;
}
bool apply_labels(Options &o) {
	if (o.preint) { printf("Error: -labels excludes -preint: a slab between two labels has no single table entry\n"); return false; }
	if (o.labels_octants && !o.labels_file.empty()) { printf("Error: -labels and -labels-octants exclude each other\n"); return false; }
	if (!o.loaded) { printf("Error: -labels needs a volume\n"); return false; }
	const uint32_t dims[3] = { ModelBase::volume.dims.x, ModelBase::volume.dims.y, ModelBase::volume.dims.z };
	const size_t voxels = (size_t) dims[0] * dims[1] * dims[2];
	std::vector<uint8_t> labels(voxels);
	if (o.labels_octants) {                   // the label of a voxel is its octant: bit 0 the upper half in x, bit 1 in y, bit 2 in z
		for (uint32_t z = 0; z < dims[2]; z++) for (uint32_t y = 0; y < dims[1]; y++) for (uint32_t x = 0; x < dims[0]; x++)
			labels[((size_t) z * dims[1] + y) * dims[0] + x] = (uint8_t) ((x >= dims[0] / 2u ? 1u : 0u) | (y >= dims[1] / 2u ? 2u : 0u) | (z >= dims[2] / 2u ? 4u : 0u));
	} else {
		FILE *f = fopen(o.labels_file.c_str(), "rb");
		const size_t got = f ? fread(labels.data(), 1, voxels, f) : 0;
		const bool more = f && fgetc(f) != EOF;
		if (f) fclose(f);
		if (got != voxels || more) { printf("Error: -labels %s does not hold the %zu bytes of the volume's dims\n", o.labels_file.c_str(), voxels); return false; }
	}
	if (!accepted(renderers[1], renderers[1]->set_labels(labels.data(), dims) != 0 || renderers[1]->set_label_table(o.label_table.data(), o.label_entries) != 0)) return false;
	renderers[1]->set_labelled(true);
	printf("Labels: %s, %u table entr%s\n", o.labels_octants ? "octants" : o.labels_file.c_str(), o.label_entries, o.label_entries == 1u ? "y" : "ies");
	return true;
}

// One row per kind, walked in this order; a kind excludes every kind above it, so each pair is refused once, by the lower one.
struct FrameKind {
	const char *flag;                           // as the messages name the kind
	bool (*given)(const Options &);
	const char *excluded;                       // the answer to a kind above it on the same line
	bool refines;                               // takes -refine
	const char *trilinear_because;              // needs -r 1, for this reason (nullptr: either renderer) ...
	bool nearest_in_benchmark;                  // ... but -b may keep -r 0, whose frames then stay composites
	bool benchmark;                             // -b is allowed
	bool (*apply)(Options &);                   // nullptr: the kind is a call of its own, not a state of the renderer
	bool (*orphans)(const Options &);           // options of this kind given without it, and the answer to them
	const char *orphaned;
};
const FrameKind kinds[] = {
	{ "-mip", [](const Options &o) { return o.mip; }, nullptr, false, nullptr, false, true, apply_mip, nullptr, nullptr },
	{ "-iso", [](const Options &o) { return o.iso; }, "Error: -iso and -mip exclude each other\n", true, "an isosurface is defined on the interpolated field", true, true, apply_iso, nullptr, nullptr },
	{ "-hybrid", [](const Options &o) { return o.hybrid; }, "Error: -hybrid excludes -mip and -iso\n", true, "its surface is defined on the interpolated field", false, true, apply_hybrid, nullptr, nullptr },
	{ "-section", [](const Options &o) { return o.section_on; }, "Error: -section excludes -mip, -iso and -hybrid\n", false, "a section is defined on the interpolated field", false, true, apply_section,
	  [](const Options &o) { return o.section_in_volume || o.section_mode_given || o.section_window_given || o.section.half_width != 0.0f; },
	  "Error: -section-half, -section-mode, -section-window and -section-in-volume need -section\n" },
	{ "-depth", [](const Options &o) { return o.depth_on; }, "Error: -depth excludes -mip, -iso, -hybrid and -section\n", false, "a depth frame is defined on the interpolated field", false, false, nullptr,
	  [](const Options &o) { return o.depth_mode_given || o.pick_on; }, "Error: -depth-mode and -pick need -depth\n" },
	{ "-labels", [](const Options &o) { return o.labels_octants || !o.labels_file.empty(); }, "Error: -labels excludes -mip, -iso, -hybrid, -section and -depth\n", false,
	  "a labelled frame is defined on the interpolated field", false, true, apply_labels, [](const Options &o) { return o.label_entries != 0u; }, "Error: -label entries need -labels or -labels-octants\n" },
};

bool apply_kinds(Options &o) {
	bool above = false;             // a kind above this one was given
	for (const FrameKind &k : kinds) {
		if (!k.given(o)) {
			if (k.orphans != nullptr && k.orphans(o)) { printf("%s", k.orphaned); return false; }
			continue;
		}
		if (!device_list.empty()) { printf("Error: %s renders on a single device (drop -devices)\n", k.flag); return false; }
		if (above) { printf("%s", k.excluded); return false; }
		if (k.refines && (o.iso_refine < 0 || o.iso_refine > 16)) { printf("Error: -refine must be in 0..16\n"); return false; }
		if (k.trilinear_because != nullptr && renderer_id != 1 && !(k.nearest_in_benchmark && o.benchmark_mode)) {
			printf("Error: %s needs the trilinear renderer (-r 1): %s\n", k.flag, k.trilinear_because); return false;
		}
		if (!k.benchmark && o.benchmark_mode) { printf("Error: %s renders single frames (drop -b)\n", k.flag); return false; }
		if (k.apply != nullptr && !k.apply(o)) return false;
		above = true;
	}
	return true;
}

// -shadow, -phong and -preint act on the composite of the trilinear renderer
bool composite_option(const Options &o, const char *flag) {
	if (o.mip || o.iso) { printf("Error: %s works with the composite (drop -mip / -iso)\n", flag); return false; }
	if (!o.benchmark_mode && renderer_id != 1) { printf("Error: %s needs the trilinear renderer (-r 1)\n", flag); return false; }
	return true;
}

// the clip, the start pose and the composite's options, in the order their announcements have
bool apply_state(const Options &o) {
	if (o.clip_box || o.clip_plane) {
		const vr_clip &clip = o.clip;
		for (int i = 0; i < PROFILER_RENDERERS; i++)
			if (!accepted(renderers[i], renderers[i]->set_clip(&clip))) return false;
		printf("Clip region:");
		if (o.clip_box) printf(" box (%g, %g, %g) - (%g, %g, %g)", clip.box_min[0], clip.box_min[1], clip.box_min[2], clip.box_max[0], clip.box_max[1], clip.box_max[2]);
		if (o.clip_plane) printf(" plane %g x + %g y + %g z + %g >= 0", clip.plane[0], clip.plane[1], clip.plane[2], clip.plane[3]);
		printf("\n");
	}
	if (!o.benchmark_mode) {
		if (o.persp) ViewBase::toggle_perspective(0);
		ViewBase::set_camera_position(make_float3(o.pose[0], o.pose[1], o.pose[2]), o.have_pose ? o.pose[3] : 3.0f);
	}
	if (o.shadow_dims != 0) {
		// the light is the view's (benchmark mode: the start view's — the reference's benchmark moves the camera, not the light); the
		// trilinear renderer only: the light grid and its factor are defined on the interpolated field
		if (!composite_option(o, "-shadow")) return false;
		vr_shadow sh;
		sh.light_pos[0] = ViewBase::view.light_pos.x; sh.light_pos[1] = ViewBase::view.light_pos.y; sh.light_pos[2] = ViewBase::view.light_pos.z;
		sh.dims = (uint32_t) o.shadow_dims; sh.step = o.shadow_step > 0.0f ? o.shadow_step : RaycasterBase::raycaster.ray_step;
		sh.strength = o.shadow_strength; sh.cutoff = 1.0f / 256.0f; sh.sampling = VR_SAMPLE_TRILINEAR;
		if (!accepted(renderers[1], renderers[1]->set_shadow(&sh))) return false;
		printf("Shadow: %d^3 nodes, light (%g, %g, %g), step %g, strength %g\n", o.shadow_dims, sh.light_pos[0], sh.light_pos[1], sh.light_pos[2], sh.step, sh.strength);
	}
	if (o.phong) {
		if (!composite_option(o, "-phong") || !accepted(renderers[1], renderers[1]->set_lighting(&o.lighting))) return false;
		printf("Lighting: ambient %g, diffuse %g, specular %g, shininess 2^%u\n", o.lighting.ambient, o.lighting.diffuse, o.lighting.specular, o.lighting.shininess_log2);
	}
	if (o.preint) {
		if (!composite_option(o, "-preint") || !accepted(renderers[1], renderers[1]->set_preintegration(true))) return false;
		printf("Classification: pre-integrated (slab)\n");
	}
	return true;
}

// the benchmark matrix, one depth frame (with its pick) or one frame; the exit status
int run(const Options &o) {
	int rc = EXIT_SUCCESS;
	if (o.benchmark_mode) {
		benchmark();
		print_profiler();
	} else if (o.depth_on) {
		std::vector<float> depth;
		if (!accepted(renderers[1], draw_depth(o.depth, depth))) return EXIT_FAILURE;
		size_t surfaces = 0;
		for (float d : depth) surfaces += d >= 0.0f ? 1u : 0u;
		printf("Depth: mode %s, opacity %g: %zu of %zu pixels carry a surface\n", depth_mode_names[o.depth.mode], o.depth.opacity, surfaces, depth.size());
		printf("%s: %dx%d depth frame in %.2f ms\n", renderers[1]->get_name(), ViewBase::view.dims.x, ViewBase::view.dims.y, Profiler::time_ms);
		if (o.pick_on) {
			vr_pick pk;
			if (!accepted(renderers[1], renderers[1]->pick(RaycasterBase::raycaster, o.depth, 1u, o.pick_xy, &pk))) rc = EXIT_FAILURE;
			else printf("Pick (%u, %u): hit %u k %.9g position (%.9g, %.9g, %.9g) voxel (%.9g, %.9g, %.9g) value %.9g alpha %.9g\n", o.pick_xy[0], o.pick_xy[1], pk.hit, pk.k,
			            pk.position[0], pk.position[1], pk.position[2], pk.voxel[0], pk.voxel[1], pk.voxel[2], pk.value, pk.alpha);
		}
		if (!o.out_ppm.empty() && write_depth_ppm(o.out_ppm.c_str(), depth) != 0) { printf("Error: cannot write %s\n", o.out_ppm.c_str()); rc = EXIT_FAILURE; }
	} else {
		draw_volume();
		printf("%s: %dx%d frame in %.2f ms\n", renderers[renderer_id]->get_name(), ViewBase::view.dims.x, ViewBase::view.dims.y, Profiler::time_ms);
		if (!o.out_ppm.empty() && write_ppm(o.out_ppm.c_str()) != 0) { printf("Error: cannot write %s\n", o.out_ppm.c_str()); rc = EXIT_FAILURE; }
	}
	return rc;
}

}  // namespace

// parse, load, create, apply the kind, apply the state, run.  Nothing is validated before the renderers exist: a refused line prints
// what the reference's start-up prints up to there.
int main(int argc, char **argv) {
	Options o;
	ViewBase::reset();
	const int ended = parse(argc, argv, o);
	if (ended >= 0) return ended;

	// VolR.cpp:412-417
	o.loaded = !o.file_name.empty() && ModelBase::load_model(o.file_name.c_str()) == 0;
	if (!o.loaded) o.loaded = use_synthetic();
	if (!o.loaded && !o.benchmark_mode) { printf("Warning: no volume data loaded (use -f or -synthetic).\n"); return EXIT_FAILURE; }
	RaycasterBase::set_view(ViewBase::view);
	RaycasterBase::reset_transfer_fn();
	if (o.loaded) RaycasterBase::set_volume(ModelBase::volume);
	Profiler::init();

	printf("Initializing renderers 0 - %d...\n", PROFILER_RENDERERS - 1);
	for (int i = 0; i < PROFILER_RENDERERS; i++)
		renderers[i] = device_list.empty() ? new HipRenderer(RaycasterBase::raycaster, device, i == 0 ? VR_SAMPLE_NEAREST : VR_SAMPLE_TRILINEAR)
		                                   : new HipRenderer(RaycasterBase::raycaster, device_list.data(), (int) device_list.size(), i == 0 ? VR_SAMPLE_NEAREST : VR_SAMPLE_TRILINEAR);
	if (!device_list.empty() && renderers[1]->ok()) printf("Frame split over %d device(s), bands gathered by %s\n", (int) device_list.size(), vr_hip_multi_transport(renderers[1]->multi()));
	for (int i = 0; i < PROFILER_RENDERERS; i++)
		if (!accepted(renderers[i], renderers[i]->ok() ? 0 : 1)) return EXIT_FAILURE;

	if (!apply_kinds(o) || !apply_state(o)) return EXIT_FAILURE;
	const int rc = run(o);
	for (int i = PROFILER_RENDERERS - 1; i >= 0; i--) delete renderers[i];      // reverse order like VolR.cpp:328-329
	return rc;
}
