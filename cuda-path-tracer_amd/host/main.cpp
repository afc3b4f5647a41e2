// hip_pt -- headless command-line front-end with the reference's flags
//   cuda_pt [--spp N] [-o out.png] <scene.json>          (reference: src/main.cpp:9-25, src/lib/configurations.cpp:7-45)
// following the call sequence of execute_cli_version (src/cli/cli.cpp:62-116): read scene, create_buffers,
// max_iterations = spp, spp x path_trace, synchronize, send_to_preview, write PNG, stage timings.
// Extra flags: --max-bounces N (the reference's cap is a compile-time 50), --denoise, --denoise-albedo, --denoise-variance [--variance-sigma S] (5s), --method, --gpu,
// --lens-radius R / --focus-distance F (the thin lens), --tonemap C / --exposure EV / --auto-exposure / --key K / --white W (the display transform), --environment FILE / --environment-scale S / --environment-size N (environment lighting; --dump-environment FILE: the decoded picture and the map, for tests, no GPU), --textures (image textures), --normal-maps (normal maps), --dump-scene FILE (flattened scene arrays, for tests; needs no GPU), --gpus N, --display final|color|normal|depth
// (DisplayBufferType of send_to_preview, path_tracer.cu:487-520: which buffer the PNG shows), --dump-raw FILE (the
// accumulated float framebuffers as they are: "PTRF", width, height, 7 as uint32, then colour rgb, normal xyz and
// depth planes as float32).  Without -o the reference opens its GLFW viewer; this build is headless and says so.
// --replay SCRIPT.json: the viewer WITHOUT a window -- App::main_loop / run_cuda (interactive-app/app.cpp:141-170) driven by
// a script of the events the reference takes from GLFW and ImGui (movement keys, right-drag, Space, the GUI's fields),
// one PNG per displayed frame (see run_replay below).
//
// --gpus N: one PROCESS per GPU (forked before anything touches HIP), rank r on device r % device_count.  The frame's
// rows are dealt to the ranks in blocks of 8 (ptc_set_interleave: sky rows are cheap, terrain rows expensive), the
// scene is replicated, nobody talks while tracing, and at the end every rank's rows go straight to rank 0 through the
// library's inter-process gather (ptc_band_export / import / publish, ptc_gather_present_rgba8: device-to-device
// copies, xGMI between GPUs).  Handles and the two barriers travel through a shared-memory page.
#include <sys/mman.h>
#include <sys/wait.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <algorithm>
#include <optional>
#include <sstream>
#include <string>
#include <vector>

#include "first_person_camera_controller.hpp"
#include "json.hpp"
#include "path_tracer.hpp"

namespace fs = std::filesystem;
using namespace hip_pt;

namespace {

struct CliConfigurations {  // configurations.hpp:11-15
  std::string filename;
  std::optional<int> spp;
  std::optional<std::string> output_filename;
  int max_bounces = 50;
  bool denoise = false;
  bool denoise_albedo = false;  // (implies denoise)
  bool denoise_variance = false;  // (implies denoise)
  float variance_sigma = 16.0f;
  bool megakernel = false;
  bool direct_light = false;
  bool environment_light = false;
  bool mis = false;
  bool smooth_normals = false;
  bool textures = false;
  bool normal_maps = false;
  int roulette = 0;
  std::optional<float> lens_radius, focus_distance;  // the thin lens (override the scene file's camera keys)
  // environment lighting (override the scene file's "environment" key, each on its own)
  std::optional<std::string> environment, dump_environment;
  std::optional<float> environment_scale;
  std::optional<int> environment_size;
  int gpu = 0;
  int gpus = 1;
  std::optional<std::string> dump_scene;
  std::optional<std::string> dump_raw;
  DisplayBufferType display = DisplayBufferType::final;
  // the display transform: the defaults are the reference display
  ptc_display_params tone{PTC_CURVE_CLAMP, 0, 1.0f, 0.18f, 4.0f, 50u, 950u};
  const char* tone_flag = nullptr;  // the first of its flags on the command line
  std::optional<std::string> replay;
  bool dry_run = false;
};

void usage()
{
  std::fprintf(stderr,
               "A Path Tracer for AMD MI355X (hip_pt; command line of cuda_pt)\nUsage:\n  hip_pt [OPTION...] <filename>\n\n"
               "  -o, --output arg     Output path tracing result to a file\n"
               "  -h, --help           Print this message\n"
               "      --spp arg        Sample per pixel (overrides the setting in the scene file)\n"
               "      --max-bounces N  bounce cap (default 50)\n"
               "      --denoise        run the A-Trous denoiser before writing the image\n"
               "      --denoise-albedo  denoise irradiance, not colour: the first-hit albedo is divided out before the filter and multiplied\n"
               "                       back after it, so that a texture's detail passes the filter (implies --denoise)\n"
               "      --denoise-variance  steer the filter's colour weight by a per-pixel variance estimate, not by one constant: low-contrast\n"
               "                       edges stay and fireflies go (implies --denoise)\n"
               "      --variance-sigma S  how many variances of colour distance that weight tolerates (default 16; finite, > 0)\n"
               "      --method M       streaming (default) | megakernel\n"
               "      --direct-light   a light sample with a shadow ray at every diffuse hit (needs --method megakernel)\n"
               "      --roulette K     Russian roulette at every bounce >= K but the last, unbiased (0 = off, the default; K in [0,64])\n"
               "      --lens-radius R  thin lens: aperture radius in world units (0 = pinhole; overrides the scene's \"lens_radius\")\n"
               "      --focus-distance F  thin lens: distance of the plane in focus, > 0 (overrides the scene's \"focus_distance\")\n"
               "      --environment-light  an environment sample with a shadow ray at every diffuse hit (needs --method megakernel;\n"
               "                       a scene whose \"environment\" says \"light\": true asks for it under --method megakernel)\n"
               "      --mis            multiple importance sampling: light samples and the path's own ray combined by the balance heuristic\n"
               "                       (needs --method megakernel and --direct-light, --environment-light or a scene that says \"light\": true)\n"
               "      --smooth-normals  shade every mesh with interpolated vertex normals, area-weighted from its triangles (needs --method\n"
               "                       megakernel; a scene that says \"smooth_normals\": true asks for it)\n"
               "      --textures       take the colour of a material that carries a \"texture\" from its picture, at the mesh's `vt` coordinates (needs\n"
               "                       --method megakernel; a scene that says \"textures\": true asks for it)\n"
               "      --normal-maps    shade a material that carries a \"normal_map\" with its picture's normals, at the mesh's `vt` coordinates (needs\n"
               "                       --method megakernel; a scene that says \"normal_maps\": true asks for it)\n"
               "      --environment FILE  environment lighting: an equirectangular Radiance .hdr (overrides the scene's \"environment\")\n"
               "      --environment-scale S  multiply the picture by S, a finite number >= 0 (default 1)\n"
               "      --environment-size N  size of the octahedral map made from it, in [2,4096] (default: the picture's height)\n"
               "      --dump-environment F  test hook: write the decoded picture and the map to F and exit (no GPU needed)\n"
               "      --gpu N          HIP device ordinal\n"
               "      --gpus N         split the frame's rows over N processes / GPUs (rank r on device r %% device count)\n"
               "      --dump-scene F   write the flattened scene to F and exit (no GPU needed)\n"
               "      --display D      buffer the image shows: final (default) | color | normal | depth\n"
               "      --tonemap C      tone curve of the final / color image: clamp (default) | reinhard | aces\n"
               "      --exposure EV    exposure in stops: every channel times 2^EV before the curve (default 0)\n"
               "      --auto-exposure  meter the image: a log-luminance histogram's trimmed mean is brought to the key\n"
               "      --key K          what --auto-exposure brings the metered level to, > 0 (default 0.18)\n"
               "      --white W        white point of --tonemap reinhard, > 0 (default 4)\n"
               "      --dump-raw F     also write the accumulated float buffers (colour, normal, depth) to F\n"
               "      --replay S.json  headless viewer: replay a script of viewer events, -o PREFIX -> PREFIX_0000.png ...\n"
               "      --dry-run        with --replay: no GPU, no images; print the camera after every event\n");
}

CliConfigurations parse_cli_args(int argc, char** argv)
{
  CliConfigurations c;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto need = [&](const char* name) -> std::string {
      if (i + 1 >= argc) {
        std::fprintf(stderr, "Option '%s' is missing an argument\n", name);
        std::exit(1);
      }
      return argv[++i];
    };
    if (a == "-h" || a == "--help") {
      usage();
      std::exit(0);
    } else if (a == "-o" || a == "--output") c.output_filename = need("output");
    else if (a.rfind("--output=", 0) == 0) c.output_filename = a.substr(9);
    else if (a == "--spp") c.spp = std::stoi(need("spp"));
    else if (a.rfind("--spp=", 0) == 0) c.spp = std::stoi(a.substr(6));
    else if (a == "--max-bounces") c.max_bounces = std::stoi(need("max-bounces"));
    else if (a == "--denoise") c.denoise = true;
    else if (a == "--denoise-albedo") c.denoise = c.denoise_albedo = true;
    else if (a == "--denoise-variance") c.denoise = c.denoise_variance = true;
    else if (a == "--variance-sigma") c.variance_sigma = std::stof(need("variance-sigma"));
    else if (a == "--method") c.megakernel = need("method") == "megakernel";
    else if (a == "--direct-light") c.direct_light = true;
    else if (a == "--environment-light") c.environment_light = true;
    else if (a == "--mis") c.mis = true;
    else if (a == "--smooth-normals") c.smooth_normals = true;
    else if (a == "--textures") c.textures = true;
    else if (a == "--normal-maps") c.normal_maps = true;
    else if (a == "--roulette") {
      // a whole decimal number in [0, 64] (ptc_set_param's range), refused here: before the scene is read or a GPU touched
      const std::string v = need("roulette");
      int k = -1;
      if (!v.empty() && v.size() <= 2 && v.find_first_not_of("0123456789") == std::string::npos) k = std::stoi(v);
      if (k < 0 || k > 64) {
        std::fprintf(stderr, "Option '--roulette': '%s' is not a number in [0,64]\n", v.c_str());
        std::exit(1);
      }
      c.roulette = k;
    }
    else if (a == "--lens-radius" || a == "--focus-distance") {
      // a finite decimal number, >= 0 (radius) or > 0 (focus distance), refused here: before the scene is read or a GPU touched
      const bool radius = a == "--lens-radius";
      const std::string v = need(a.c_str() + 2);
      char* end = nullptr;
      const float x = std::strtof(v.c_str(), &end);
      if (v.empty() || *end != '\0' || !std::isfinite(x) || x < 0.0f || (!radius && x == 0.0f)) {
        std::fprintf(stderr, "Option '%s': '%s' is not a finite number %s\n", a.c_str(), v.c_str(), radius ? ">= 0" : "> 0");
        std::exit(1);
      }
      (radius ? c.lens_radius : c.focus_distance) = x;
    }
    else if (a == "--environment") c.environment = need("environment");
    else if (a == "--dump-environment") c.dump_environment = need("dump-environment");
    else if (a == "--environment-scale") {
      const std::string v = need("environment-scale");
      char* end = nullptr;
      const float x = std::strtof(v.c_str(), &end);
      if (v.empty() || *end != '\0' || !std::isfinite(x) || x < 0.0f) {
        std::fprintf(stderr, "Option '--environment-scale': '%s' is not a finite number >= 0\n", v.c_str());
        std::exit(1);
      }
      c.environment_scale = x;
    }
    else if (a == "--environment-size") {
      const std::string v = need("environment-size");
      int n = -1;
      if (!v.empty() && v.size() <= 4 && v.find_first_not_of("0123456789") == std::string::npos) n = std::stoi(v);
      if (n < 2 || n > 4096) {
        std::fprintf(stderr, "Option '--environment-size': '%s' is not a number in [2,4096]\n", v.c_str());
        std::exit(1);
      }
      c.environment_size = n;
    }
    else if (a == "--tonemap") {
      // the display transform's flags are refused here: before the scene is read or a GPU touched
      const std::string v = need("tonemap");
      if (v == "clamp") c.tone.curve = PTC_CURVE_CLAMP;
      else if (v == "reinhard") c.tone.curve = PTC_CURVE_REINHARD;
      else if (v == "aces") c.tone.curve = PTC_CURVE_ACES;
      else {
        std::fprintf(stderr, "Option '--tonemap': unknown curve '%s' (clamp, reinhard, aces)\n", v.c_str());
        std::exit(1);
      }
      if (!c.tone_flag) c.tone_flag = "--tonemap";
    }
    else if (a == "--auto-exposure") {
      c.tone.metering = 1;
      if (!c.tone_flag) c.tone_flag = "--auto-exposure";
    }
    else if (a == "--exposure" || a == "--white" || a == "--key") {
      const std::string v = need(a.c_str() + 2);
      char* end = nullptr;
      const double x = std::strtod(v.c_str(), &end);
      const bool stops = a == "--exposure";
      const float f = stops ? (float)std::exp2(x) : (float)x;  // (stops so far from 0 that 2^EV is 0 or infinite in binary32 are refused too)
      if (v.empty() || *end != '\0' || !std::isfinite(x) || !std::isfinite(f) || !(f > 0.0f)) {
        std::fprintf(stderr, "Option '%s': '%s' is not a finite number%s\n", a.c_str(), v.c_str(), stops ? " of stops in binary32's range" : " > 0");
        std::exit(1);
      }
      (stops ? c.tone.exposure : a == "--white" ? c.tone.white : c.tone.key) = f;
      if (!c.tone_flag) c.tone_flag = stops ? "--exposure" : a == "--white" ? "--white" : "--key";
    }
    else if (a == "--gpu") c.gpu = std::stoi(need("gpu"));
    else if (a == "--gpus") c.gpus = std::stoi(need("gpus"));
    else if (a == "--dump-scene") c.dump_scene = need("dump-scene");
    else if (a == "--dump-raw") c.dump_raw = need("dump-raw");
    else if (a == "--replay") c.replay = need("replay");
    else if (a == "--dry-run") c.dry_run = true;
    else if (a == "--display") {
      const std::string d = need("display");
      if (d == "final") c.display = DisplayBufferType::final;
      else if (d == "color") c.display = DisplayBufferType::color;
      else if (d == "normal") c.display = DisplayBufferType::normal;
      else if (d == "depth") c.display = DisplayBufferType::depth;
      else {
        std::fprintf(stderr, "Option '--display': unknown buffer '%s' (final, color, normal, depth)\n", d.c_str());
        std::exit(1);
      }
    }
    else if (!a.empty() && a[0] == '-') {
      std::fprintf(stderr, "Option '%s' does not exist\n", a.c_str());
      std::exit(1);
    } else c.filename = a;
  }
  if (c.direct_light && !c.megakernel) {  // before any GPU is touched: the streaming loop would render without it
    std::fprintf(stderr, "hip_pt: --direct-light needs --method megakernel (the streaming method renders no direct light)\n");
    std::exit(1);
  }
  if (c.environment_light && !c.megakernel) {  // ... and no environment light
    std::fprintf(stderr, "hip_pt: --environment-light needs --method megakernel (the streaming method renders no direct light)\n");
    std::exit(1);
  }
  if (c.mis && !c.megakernel) {  // ... and nothing to combine
    std::fprintf(stderr, "hip_pt: --mis needs --method megakernel (the streaming method renders no direct light)\n");
    std::exit(1);
  }
  if (c.smooth_normals && !c.megakernel) {  // ... and shades with face normals
    std::fprintf(stderr, "hip_pt: --smooth-normals needs --method megakernel (the streaming method shades with face normals)\n");
    std::exit(1);
  }
  if (c.textures && !c.megakernel) {  // ... and its hit records carry no primitive
    std::fprintf(stderr, "hip_pt: --textures needs --method megakernel (the streaming method's hit records carry no primitive)\n");
    std::exit(1);
  }
  if (c.normal_maps && !c.megakernel) {
    std::fprintf(stderr, "hip_pt: --normal-maps needs --method megakernel (the streaming method's hit records carry no primitive)\n");
    std::exit(1);
  }
  if (c.tone_flag && (c.display == DisplayBufferType::normal || c.display == DisplayBufferType::depth)) {
    std::fprintf(stderr, "hip_pt: %s applies to radiance: not with --display normal or depth (the display transform leaves those views alone)\n",
                 c.tone_flag);
    std::exit(1);
  }
  if (c.filename.empty()) {
    std::fprintf(stderr, "Usage: hip_pt [options] <filename>\nRun 'hip_pt --help' for more information");
    std::exit(1);
  }
  return c;
}

// assets/assets.cpp:6-22: the OUTERMOST ancestor of the working directory that contains "assets/"
std::optional<fs::path> locate_asset_path(const fs::path& current_path)
{
  std::optional<fs::path> result;
  for (auto path = current_path; path != current_path.root_path(); path = path.parent_path()) {
    const auto assets_path = path / "assets";
    if (fs::exists(assets_path) && fs::is_directory(assets_path)) result = assets_path;
  }
  return result;
}

class Stopwatch {  // cli.cpp:27-60
  using clock = std::chrono::steady_clock;
  clock::time_point start_ = clock::now(), last_ = clock::now();
  std::vector<std::pair<std::string, double>> entries_;

public:
  void end_stage(std::string name)
  {
    const auto now = clock::now();
    entries_.emplace_back(std::move(name), std::chrono::duration<double>(now - last_).count());
    last_ = now;
  }
  void report() const
  {
    std::printf("Elapsed time\n===========\n");
    for (const auto& [name, s] : entries_) std::printf("%s: %gs\n", name.c_str(), s);
    std::printf("Total: %gs\n", std::chrono::duration<double>(last_ - start_).count());
  }
};

template <typename T>
void dump_vec(std::ofstream& out, const std::vector<T>& v)
{
  const uint64_t n = v.size();
  out.write(reinterpret_cast<const char*>(&n), 8);
  out.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(n * sizeof(T)));
}

// --dump-raw: the float framebuffers as they are.  fetch(which, dst) fills width*height*{3,3,1} floats.
template <typename Fetch>
bool write_raw(const std::string& path, uint32_t width, uint32_t height, Fetch fetch)
{
  std::ofstream out(path, std::ios::binary);
  if (!out) return false;
  const uint32_t head[3] = {width, height, 7u};
  out.write("PTRF", 4);
  out.write(reinterpret_cast<const char*>(head), sizeof head);
  std::vector<float> plane((size_t)width * height * 3u);
  const int which[3] = {PTC_BUF_COLOR, PTC_BUF_NORMAL, PTC_BUF_DEPTH};
  for (int k = 0; k < 3; ++k) {
    const size_t floats = (size_t)width * height * (which[k] == PTC_BUF_DEPTH ? 1u : 3u);
    fetch(which[k], plane.data());
    out.write(reinterpret_cast<const char*>(plane.data()), (std::streamsize)(floats * sizeof(float)));
  }
  return (bool)out;
}

// ---- --replay: the interactive front-end without a window ---------------------------------------------------
// What App does (interactive-app/app.cpp): own a PathTracer and a FirstPersonCameraController on the scene's camera
// (:16-19), max_iterations = the scene's spp and buffers of the WINDOW's size, 800 x 800 (:36,127-131); then per loop
// turn (:162-170) poll the events -- a movement key or a right-drag moves the camera and restarts the accumulation
// (:64-67,108-113), Space restarts (:56), a resize reallocates (:45) -- run_cuda (:141-160: path_trace [+ denoise] +
// synchronise, repeated for 16 ms, then send_to_preview of the chosen DisplayBufferType), and let the GUI edit
// max_iterations, the method, the denoiser and the display (gui.cpp:84-108).  The script is those events:
//   {"window": [w, h], "iterations_per_frame": 2, "events": [
//      {"frames": 3},                      loop turns: run_cuda + one PNG each
//      {"key": "W", "count": 5},           GLFW_REPEAT of W/A/S/D/R/F            {"mouse": [dx, dy]}   right-drag, pixels
//      {"space": true}  {"resize": [w, h]}  {"denoise": true}  {"denoise_albedo": true}  {"denoise_variance": true}  {"display": "normal"}  {"method": "megakernel"}
//      {"max_iterations": 64}  {"filter_size": 10}  {"speed": 0.5}  {"position": [x, y, z]}  {"reset": true} ]}
// A turn runs "iterations_per_frame" iterations (default 1) instead of as many as fit into 16 ms, so that a replay
// gives the same frames every time; "budget_ms": 16 restores the reference's clock.
int run_replay(const CliConfigurations& configs, SceneDescription& scene_desc)
{
  std::ifstream file(*configs.replay);
  if (!file) throw std::runtime_error("Cannot open replay script " + *configs.replay);
  std::stringstream text;
  text << file.rdbuf();
  const JsonPtr root = JsonReader(text.str()).parse();
  UResolution resolution{800u, 800u};  // app.cpp:36
  if (const Json* w = root->find("window")) resolution = {(unsigned)w->arr.at(0)->f(), (unsigned)w->arr.at(1)->f()};
  const int per_frame = root->find("iterations_per_frame") ? (int)root->at("iterations_per_frame").f() : 1;
  const double budget_ms = root->find("budget_ms") ? root->at("budget_ms").f() : 0.0;

  Camera& camera = scene_desc.camera;
  FirstPersonCameraController controller{camera};  // app.cpp:18 (reset(): the camera is re-expressed as yaw + pitch)
  if (configs.dry_run) {  // the controller alone (no GPU): one line per event
    std::printf("start: position %.9g %.9g %.9g yaw %.9g pitch %.9g rotation %.9g %.9g %.9g %.9g\n", camera.position[0], camera.position[1],
                camera.position[2], controller.yaw(), controller.pitch(), camera.rotation_wxyz[0], camera.rotation_wxyz[1],
                camera.rotation_wxyz[2], camera.rotation_wxyz[3]);
    int restarts = 0;
    for (const JsonPtr& ev : root->at("events").arr) {
      bool moved = false;
      if (const Json* j = ev->find("key")) {
        const int count = ev->find("count") ? (int)ev->at("count").f() : 1;
        for (int i = 0; i < count; ++i) moved = (!j->str.empty() && controller.on_key_press(j->str[0])) || moved;
      } else if (const Json* j = ev->find("mouse")) {
        const float rad = 0.01745329251994329576923690768489f;
        moved = controller.on_mouse_move(rad * j->arr.at(0)->f(), rad * j->arr.at(1)->f());
      } else if (const Json* j = ev->find("speed")) {
        controller.speed = j->f();
      } else if (const Json* j = ev->find("position")) {
        controller.set_position(j->arr.at(0)->f(), j->arr.at(1)->f(), j->arr.at(2)->f());
        controller.update_camera();
        moved = true;
      } else if (ev->find("reset")) {
        controller.reset();
        moved = true;
      } else {
        continue;
      }
      restarts += moved ? 1 : 0;
      std::printf("event: position %.9g %.9g %.9g yaw %.9g pitch %.9g rotation %.9g %.9g %.9g %.9g restarts %d\n", camera.position[0],
                  camera.position[1], camera.position[2], controller.yaw(), controller.pitch(), camera.rotation_wxyz[0],
                  camera.rotation_wxyz[1], camera.rotation_wxyz[2], camera.rotation_wxyz[3], restarts);
    }
    return 0;
  }
  PathTracer path_tracer{configs.gpu};
  path_tracer.max_bounces = configs.max_bounces;
  path_tracer.max_iterations = scene_desc.spp;      // app.cpp:130
  path_tracer.smooth_normals = configs.smooth_normals || scene_desc.smooth_normals;  // (before create_buffers, which computes the normals)
  path_tracer.textures = configs.textures || scene_desc.textures;  // (create_buffers sets the scene's textures and coordinates)
  path_tracer.normal_maps = configs.normal_maps || scene_desc.normal_maps;  // (... and its normal-map binding)
  path_tracer.create_buffers(resolution, scene_desc);
  bool enable_denoising = configs.denoise;
  path_tracer.denoise_albedo = configs.denoise_albedo;
  path_tracer.denoise_variance = configs.denoise_variance;
  path_tracer.denoise_variance_sigma = configs.variance_sigma;
  DisplayBufferType display = configs.display;
  if (configs.megakernel) path_tracer.current_gpu_method = GPUMethod::megakernel;
  path_tracer.direct_light = configs.direct_light;
  // (the flag, or the scene's "environment": {"light": true} where the method renders it)
  path_tracer.environment_light = configs.environment_light || (configs.megakernel && scene_desc.environment_source.light);
  path_tracer.mis = configs.mis;
  path_tracer.roulette = configs.roulette;
  if (scene_desc.camera.lens_radius > 0.0f) path_tracer.lens = {scene_desc.camera.lens_radius, scene_desc.camera.focus_distance};
  path_tracer.display = configs.tone;
  path_tracer.environment = scene_desc.environment;

  int shown = 0;
  std::vector<uchar4> buffer;
  auto turn = [&]() {  // run_cuda, app.cpp:141-160
    const auto start = std::chrono::steady_clock::now();
    int done = 0;
    do {
      path_tracer.path_trace(camera, resolution);
      if (enable_denoising) path_tracer.denoise(resolution);
      path_tracer.synchronize();
      ++done;
    } while (budget_ms > 0.0 ? std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - start).count() < budget_ms
                             : done < per_frame);
    buffer.resize((size_t)resolution.width * resolution.height);
    path_tracer.send_to_preview(buffer.data(), resolution, display);
    char name[32];
    std::snprintf(name, sizeof name, "_%04d.png", shown++);
    if (!write_png(*configs.output_filename + name, (int)resolution.width, (int)resolution.height, buffer.data()))
      throw std::runtime_error("Failed to write " + *configs.output_filename + name);
  };
  for (const JsonPtr& ev : root->at("events").arr) {
    if (const Json* j = ev->find("frames")) {
      for (int i = 0, n = (int)j->f(); i < n; ++i) turn();
    } else if (const Json* j = ev->find("key")) {
      const int count = ev->find("count") ? (int)ev->at("count").f() : 1;
      for (int i = 0; i < count; ++i)
        if (!j->str.empty() && controller.on_key_press(j->str[0])) path_tracer.restart();  // app.cpp:64-67
    } else if (const Json* j = ev->find("mouse")) {
      const float rad = 0.01745329251994329576923690768489f;  // glm::radians, app.cpp:110-111
      if (controller.on_mouse_move(rad * j->arr.at(0)->f(), rad * j->arr.at(1)->f())) path_tracer.restart();
    } else if (ev->find("space")) {
      path_tracer.restart();  // app.cpp:56
    } else if (const Json* j = ev->find("resize")) {
      resolution = {(unsigned)j->arr.at(0)->f(), (unsigned)j->arr.at(1)->f()};
      path_tracer.resize_image(resolution);  // app.cpp:45
    } else if (const Json* j = ev->find("denoise")) {
      enable_denoising = j->b;
    } else if (const Json* j = ev->find("denoise_albedo")) {  // (no reference equivalent: the denoiser's albedo factorisation)
      path_tracer.denoise_albedo = j->b;
    } else if (const Json* j = ev->find("denoise_variance")) {  // (no reference equivalent: the variance-guided passes)
      path_tracer.denoise_variance = j->b;
    } else if (const Json* j = ev->find("display")) {
      display = j->str == "color" ? DisplayBufferType::color : j->str == "normal" ? DisplayBufferType::normal
                : j->str == "depth" ? DisplayBufferType::depth : DisplayBufferType::final;
    } else if (const Json* j = ev->find("method")) {
      path_tracer.current_gpu_method = j->str == "megakernel" ? GPUMethod::megakernel : GPUMethod::streaming;
    } else if (const Json* j = ev->find("max_iterations")) {
      path_tracer.max_iterations = std::max(1, (int)j->f());  // gui.cpp:103-104
    } else if (const Json* j = ev->find("filter_size")) {
      path_tracer.atrous_denoiser.filter_size = (int)j->f();
    } else if (const Json* j = ev->find("speed")) {
      controller.speed = j->f();
    } else if (const Json* j = ev->find("position")) {  // the camera panel's "Translation" field, first_person_camera_controller.cpp:121-126
      controller.set_position(j->arr.at(0)->f(), j->arr.at(1)->f(), j->arr.at(2)->f());
      controller.update_camera();
      path_tracer.restart();
    } else if (ev->find("reset")) {
      controller.reset();
      path_tracer.restart();
    } else {
      throw std::runtime_error("replay: unknown event");
    }
  }
  const ptc_stats st = path_tracer.stats();
  std::printf("replayed %s: %d frames shown, %llu rays, camera at (%g, %g, %g) yaw %g pitch %g\n", configs.replay->c_str(), shown,
              (unsigned long long)st.rays_total, camera.position[0], camera.position[1], camera.position[2], controller.yaw(),
              controller.pitch());
  return 0;
}

// ---- --gpus N -------------------------------------------------------------------------------------------------
constexpr int kMaxRanks = 64;
constexpr uint32_t kBlockRows = 8;
struct Shared {  // one MAP_SHARED page set up before the fork
  std::atomic<uint32_t> arrived;
  std::atomic<uint32_t> generation;
  std::atomic<int> failed;
  ptc_band_handle handles[kMaxRanks];
  unsigned long long rays[kMaxRanks];
};

// all ranks meet; false when a rank has failed or nothing happens for two minutes
bool barrier(Shared* sh, int n)
{
  const uint32_t gen = sh->generation.load();
  if (sh->arrived.fetch_add(1u) + 1u == (uint32_t)n) {
    sh->arrived.store(0u);
    sh->generation.fetch_add(1u);
    return sh->failed.load() == 0;
  }
  for (int waited_ms = 0; sh->generation.load() == gen; ++waited_ms) {
    if (sh->failed.load() != 0 || waited_ms > 120000) return false;
    usleep(1000);
  }
  return sh->failed.load() == 0;
}

int run_rank(const CliConfigurations& configs, const SceneDescription& scene_desc, Shared* sh, int rank, int world)
try {
  int devices = 0;
  if (ptc_device_count(&devices) < 0 || devices <= 0) throw std::runtime_error("no HIP device");
  const UResolution resolution{(unsigned)scene_desc.resolution[0], (unsigned)scene_desc.resolution[1]};
  const int spp = scene_desc.spp;
  Stopwatch stopwatch;
  PathTracer path_tracer{rank % devices};
  path_tracer.max_bounces = configs.max_bounces;
  if (configs.megakernel) path_tracer.current_gpu_method = GPUMethod::megakernel;
  path_tracer.direct_light = configs.direct_light;
  // (the flag, or the scene's "environment": {"light": true} where the method renders it)
  path_tracer.environment_light = configs.environment_light || (configs.megakernel && scene_desc.environment_source.light);
  path_tracer.mis = configs.mis;
  path_tracer.smooth_normals = configs.smooth_normals || scene_desc.smooth_normals;  // (before create_buffers, which computes the normals)
  path_tracer.textures = configs.textures || scene_desc.textures;  // (create_buffers sets the scene's textures and coordinates)
  path_tracer.normal_maps = configs.normal_maps || scene_desc.normal_maps;  // (... and its normal-map binding)
  path_tracer.roulette = configs.roulette;
  if (scene_desc.camera.lens_radius > 0.0f) path_tracer.lens = {scene_desc.camera.lens_radius, scene_desc.camera.focus_distance};
  path_tracer.display = configs.tone;
  path_tracer.environment = scene_desc.environment;
  path_tracer.create_buffers(resolution, scene_desc);
  auto check = [&](int rc, const char* what) {
    if (rc < 0) throw std::runtime_error(std::string(what) + ": " + ptc_last_error(path_tracer.handle()));
  };
  check(ptc_set_interleave(path_tracer.handle(), (uint32_t)rank, (uint32_t)world, kBlockRows), "set_interleave");
  // every rank numbers its paths from 0: an offset keeps the ranks' random streams apart (path_tracer.cu:300)
  check(ptc_set_param(path_tracer.handle(), "slot_offset", (int)((unsigned)rank * resolution.width * resolution.height)), "slot_offset");
  if (rank != 0) check(ptc_band_export(path_tracer.handle(), &sh->handles[rank]), "band_export");
  path_tracer.synchronize();
  if (!barrier(sh, world)) throw std::runtime_error("another rank failed during set-up");
  if (rank == 0) {
    for (int r = 1; r < world; ++r) check(ptc_band_import(path_tracer.handle(), (uint32_t)r, &sh->handles[r]), "band_import");
    std::printf("Start path tracing\nspp: %d\nwidth: %u, height: %u\nranks: %d on %d device(s)\n", spp, resolution.width,
                resolution.height, world, devices);
  }
  stopwatch.end_stage("Initialization");
  path_tracer.max_iterations = spp;
  for (int i = 0; i < spp; ++i) path_tracer.path_trace(scene_desc.camera, resolution);
  // the rows the image will show (ptc_gather_present_rgba8 gathers the buffer of its display type)
  const int shown = configs.display == DisplayBufferType::normal ? PTC_BUF_NORMAL
                    : configs.display == DisplayBufferType::depth ? PTC_BUF_DEPTH : PTC_BUF_COLOR;
  if (rank != 0) check(ptc_band_publish(path_tracer.handle(), shown), "band_publish");
  else path_tracer.synchronize();
  sh->rays[rank] = path_tracer.stats().rays_total;
  if (!barrier(sh, world)) throw std::runtime_error("another rank failed while tracing");
  stopwatch.end_stage("Path Tracing");
  if (rank == 0) {
    std::vector<uchar4> buffer((size_t)resolution.width * resolution.height);
    check(ptc_set_display(path_tracer.handle(), &configs.tone), "display");  // the root meters the whole gathered frame
    check(ptc_gather_present_rgba8(path_tracer.handle(), buffer.data(), 0, static_cast<int>(configs.display)), "gather_present");
    const fs::path output_path{*configs.output_filename};
    if (output_path.extension() == ".png") {
      if (!write_png(output_path.string(), (int)resolution.width, (int)resolution.height, buffer.data()))
        std::fprintf(stderr, "Failed to write to image file %s\n", output_path.string().c_str());
    } else {
      std::fprintf(stderr, "%s has an unrecognized extension\n", output_path.string().c_str());
    }
    stopwatch.end_stage("Gather + write image file");
  }
  if (configs.dump_raw) {  // every buffer is one more publish / gather round
    const int which[3] = {PTC_BUF_COLOR, PTC_BUF_NORMAL, PTC_BUF_DEPTH};
    std::vector<std::vector<float>> planes(3);
    for (int k = 0; k < 3; ++k) {
      if (!barrier(sh, world)) throw std::runtime_error("another rank failed");  // the root has pulled the previous rows
      if (rank != 0) check(ptc_band_publish(path_tracer.handle(), which[k]), "band_publish");
      if (!barrier(sh, world)) throw std::runtime_error("another rank failed while publishing");
      if (rank == 0) {
        planes[k].resize((size_t)resolution.width * resolution.height * (which[k] == PTC_BUF_DEPTH ? 1u : 3u));
        check(ptc_gather_frame(path_tracer.handle(), which[k], planes[k].data(), 0), "gather_frame");
      }
    }
    if (rank == 0) {
      int k = 0;
      if (!write_raw(*configs.dump_raw, resolution.width, resolution.height,
                     [&](int, float* dst) { std::memcpy(dst, planes[k].data(), planes[k].size() * sizeof(float)); ++k; }))
        std::fprintf(stderr, "Failed to write %s\n", configs.dump_raw->c_str());
    }
  }
  if (!barrier(sh, world)) throw std::runtime_error("another rank failed at the end");  // peers keep their rows until here
  if (rank == 0) {
    unsigned long long rays = 0;
    for (int r = 0; r < world; ++r) rays += sh->rays[r];
    std::printf("Done path tracing %s!\n\n", scene_desc.filename.c_str());
    stopwatch.report();
    std::printf("rays: %llu over %d ranks\n", rays, world);
  }
  return 0;
} catch (const std::exception& e) {
  sh->failed.store(1);
  std::fprintf(stderr, "hip_pt rank %d fatal error: %s\n", rank, e.what());
  return 1;
}

int run_ranks(const CliConfigurations& configs, const SceneDescription& scene_desc)
{
  const int world = configs.gpus;
  if (world > kMaxRanks) {
    std::fprintf(stderr, "hip_pt: at most %d ranks\n", kMaxRanks);
    return 1;
  }
  // (the megakernel seeds by frame pixel, so its ranks render the single-GPU image; it is let through for --direct-light,
  // --environment-light, --mis, --smooth-normals, --textures and --normal-maps, which the streaming method cannot render)
  if (configs.denoise ||
      (configs.megakernel && !configs.direct_light && !configs.environment_light && !configs.mis && !configs.smooth_normals && !scene_desc.smooth_normals &&
       !configs.textures && !scene_desc.textures && !configs.normal_maps && !scene_desc.normal_maps)) {
    std::fprintf(stderr, "hip_pt: --gpus N renders in streaming mode without the denoiser (it needs the whole frame in one context)\n");
    return 1;
  }
  void* page = mmap(nullptr, sizeof(Shared), PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
  if (page == MAP_FAILED) {
    std::perror("mmap");
    return 1;
  }
  Shared* sh = new (page) Shared{};
  std::fflush(stdout);
  std::fflush(stderr);
  std::vector<pid_t> children;
  for (int r = 0; r < world; ++r) {
    const pid_t pid = fork();  // nothing in this process has touched HIP yet
    if (pid < 0) {
      std::perror("fork");
      sh->failed.store(1);
      break;
    }
    if (pid == 0) {
      const int rc = run_rank(configs, scene_desc, sh, r, world);
      std::fflush(stdout);
      std::fflush(stderr);
      _exit(rc);
    }
    children.push_back(pid);
  }
  int rc = sh->failed.load() ? 1 : 0;
  for (pid_t pid : children) {
    int status = 0;
    if (waitpid(pid, &status, 0) < 0 || !WIFEXITED(status) || WEXITSTATUS(status) != 0) rc = 1;
  }
  munmap(page, sizeof(Shared));
  return rc;
}

}  // namespace

int main(int argc, char** argv)
try {
  const CliConfigurations configs = parse_cli_args(argc, argv);
  Stopwatch stopwatch;

  // read_scene, assets/scene_parser.cpp:6-25: asset_path / filename (a path that exists as given is used as is)
  fs::path path = configs.filename;
  if (!fs::exists(path)) {
    const auto assets = locate_asset_path(fs::current_path());
    if (!assets) {
      std::fprintf(stderr, "Panic: Cannot find assets directory\n");
      return 1;
    }
    path = *assets / configs.filename;
  }
  path = fs::canonical(path);
  if (path.extension() != ".json") {
    std::fprintf(stderr, "Panic: Unsupported file extension %s!\n", path.extension().string().c_str());
    return 1;
  }
  SceneDescription scene_desc = scene_from_json(path.string(), /*read_environment*/ false);  // (the picture: below, once)
  scene_desc.filename = configs.filename;
  if (configs.spp) scene_desc.spp = *configs.spp;
  // a scene that asks for smooth normals needs the method that renders them (before any GPU is touched)
  if (scene_desc.smooth_normals && !configs.megakernel) {
    std::fprintf(stderr, "hip_pt: the scene says \"smooth_normals\": true, which needs --method megakernel (the streaming method shades with face normals)\n");
    return 1;
  }
  // ... and so does a scene that asks for textures, or whose materials carry one
  if ((scene_desc.textures || scene_desc.has_textures()) && !configs.megakernel) {
    std::fprintf(stderr, "hip_pt: the scene %s, which needs --method megakernel (the streaming method's hit records carry no primitive)\n",
                 scene_desc.textures ? "says \"textures\": true" : "has a material with a \"texture\"");
    return 1;
  }
  if ((scene_desc.normal_maps || scene_desc.has_normal_maps()) && !configs.megakernel) {
    std::fprintf(stderr, "hip_pt: the scene %s, which needs --method megakernel (the streaming method's hit records carry no primitive)\n",
                 scene_desc.normal_maps ? "says \"normal_maps\": true" : "has a material with a \"normal_map\"");
    return 1;
  }
  // --mis combines light samples with the path: it needs a light that is sampled (before any GPU is touched)
  if (configs.mis && !configs.direct_light && !configs.environment_light && !scene_desc.environment_source.light) {
    std::fprintf(stderr, "hip_pt: --mis needs --direct-light, --environment-light or a scene whose \"environment\" says \"light\": true\n");
    return 1;
  }
  // the thin lens: the command line over the scene file; a radius > 0 needs a focus distance from one of them (before any GPU is touched)
  if (configs.lens_radius) scene_desc.camera.lens_radius = *configs.lens_radius;
  if (configs.focus_distance) scene_desc.camera.focus_distance = *configs.focus_distance;
  if (scene_desc.camera.lens_radius > 0.0f && !(scene_desc.camera.focus_distance > 0.0f)) {
    std::fprintf(stderr, "hip_pt: a lens radius > 0 needs a focus distance (--focus-distance F, or \"focus_distance\" in the scene's camera)\n");
    return 1;
  }
  // environment lighting: the command line over the scene file, value by value; the one picture that counts is read here, once
  // (before any GPU is touched) -- a scene's own picture that the command line replaces is not opened
  if ((configs.environment_scale || configs.environment_size) && !configs.environment && scene_desc.environment_source.file.empty()) {
    std::fprintf(stderr, "hip_pt: --environment-scale / --environment-size need an environment (--environment FILE, or \"environment\" in the scene)\n");
    return 1;
  }
  HdrImage environment_picture;
  {
    auto& src = scene_desc.environment_source;
    if (configs.environment) src.file = *configs.environment;
    if (configs.environment_scale) src.scale = *configs.environment_scale;
    if (configs.environment_size) src.size = *configs.environment_size;
    if (!src.file.empty()) scene_desc.environment = load_environment(src.file, src.scale, src.size, &environment_picture);
  }
  if (configs.dump_environment) {
    if (!scene_desc.environment) {
      std::fprintf(stderr, "hip_pt: --dump-environment needs an environment (--environment FILE, or \"environment\" in the scene)\n");
      return 1;
    }
    std::ofstream out(*configs.dump_environment, std::ios::binary);
    const int32_t dims[2] = {environment_picture.width, environment_picture.height};
    out.write(reinterpret_cast<const char*>(dims), sizeof dims);
    dump_vec(out, environment_picture.rgb);
    dump_vec(out, scene_desc.environment->rgb);
    return 0;
  }
  stopwatch.end_stage("Scene loading");

  if (configs.dump_scene) {
    const FlatScene flat = scene_desc.build_scene();
    std::ofstream out(*configs.dump_scene, std::ios::binary);
    dump_vec(out, flat.objects);
    dump_vec(out, flat.object_material_indices);
    dump_vec(out, flat.spheres);
    dump_vec(out, flat.materials);
    dump_vec(out, flat.positions);
    dump_vec(out, flat.indices);
    const ptc_camera cam = scene_desc.camera.to_c();
    out.write(reinterpret_cast<const char*>(&cam), sizeof cam);
    const int32_t tail[3] = {scene_desc.resolution[0], scene_desc.resolution[1], scene_desc.spp};
    out.write(reinterpret_cast<const char*>(tail), sizeof tail);
    if (scene_desc.camera.lens_radius != 0.0f || scene_desc.camera.focus_distance != 0.0f) {  // (a scene without a lens: the dump as ever)
      const float lens[2] = {scene_desc.camera.lens_radius, scene_desc.camera.focus_distance};
      out.write(reinterpret_cast<const char*>(lens), sizeof lens);
    }
    if (!flat.texcoords.empty() || !flat.textures.empty()) {  // (a scene without textures: the dump as ever)
      const char tag[4] = {'T', 'E', 'X', '0'};
      out.write(tag, sizeof tag);
      dump_vec(out, flat.texcoords);
      dump_vec(out, flat.material_texture);
      const uint64_t count = flat.textures.size();
      out.write(reinterpret_cast<const char*>(&count), sizeof count);
      for (const TextureSource& t : flat.textures) {
        const PngImage img = read_png(t.file);
        const uint32_t head[5] = {(uint32_t)img.width, (uint32_t)img.height, t.encoding, t.filter, t.wrap};
        out.write(reinterpret_cast<const char*>(head), sizeof head);
        dump_vec(out, img.rgba);
      }
      if (!flat.material_normal_map.empty()) {  // (a scene without normal maps: the dump as ever)
        const char maps[4] = {'N', 'M', 'P', '0'};
        out.write(maps, sizeof maps);
        dump_vec(out, flat.material_normal_map);
      }
    }
    return 0;
  }
  if (configs.replay && configs.dry_run) return run_replay(configs, scene_desc);
  if (!configs.output_filename) {
    std::fprintf(stderr, "hip_pt: this build is headless (no GLFW viewer); give -o <file.png>, or --replay <script.json> -o <prefix>\n");
    return 1;
  }

  if (configs.replay) return run_replay(configs, scene_desc);
  if (configs.gpus > 1) return run_ranks(configs, scene_desc);

  const UResolution resolution{(unsigned)scene_desc.resolution[0], (unsigned)scene_desc.resolution[1]};
  const int spp = scene_desc.spp;
  PathTracer path_tracer{configs.gpu};
  path_tracer.max_bounces = configs.max_bounces;
  if (configs.megakernel) path_tracer.current_gpu_method = GPUMethod::megakernel;
  path_tracer.direct_light = configs.direct_light;
  // (the flag, or the scene's "environment": {"light": true} where the method renders it)
  path_tracer.environment_light = configs.environment_light || (configs.megakernel && scene_desc.environment_source.light);
  path_tracer.mis = configs.mis;
  path_tracer.smooth_normals = configs.smooth_normals || scene_desc.smooth_normals;  // (before create_buffers, which computes the normals)
  path_tracer.textures = configs.textures || scene_desc.textures;  // (create_buffers sets the scene's textures and coordinates)
  path_tracer.normal_maps = configs.normal_maps || scene_desc.normal_maps;  // (... and its normal-map binding)
  path_tracer.roulette = configs.roulette;
  path_tracer.denoise_albedo = configs.denoise_albedo;
  path_tracer.denoise_variance = configs.denoise_variance;
  path_tracer.denoise_variance_sigma = configs.variance_sigma;
  if (scene_desc.camera.lens_radius > 0.0f) path_tracer.lens = {scene_desc.camera.lens_radius, scene_desc.camera.focus_distance};
  path_tracer.display = configs.tone;
  path_tracer.environment = scene_desc.environment;
  path_tracer.create_buffers(resolution, scene_desc);
  path_tracer.synchronize();
  std::printf("Start path tracing\nspp: %d\nwidth: %u, height: %u\n", spp, resolution.width, resolution.height);
  stopwatch.end_stage("Initialization");

  path_tracer.max_iterations = spp;
  for (int i = 0; i < spp; ++i) path_tracer.path_trace(scene_desc.camera, resolution);
  if (configs.denoise) path_tracer.denoise(resolution);
  path_tracer.synchronize();
  stopwatch.end_stage("Path Tracing");

  std::vector<uchar4> buffer((size_t)resolution.width * resolution.height);
  path_tracer.send_to_preview(buffer.data(), resolution, configs.display);
  const fs::path output_path{*configs.output_filename};
  if (output_path.extension() == ".png") {
    if (!write_png(output_path.string(), (int)resolution.width, (int)resolution.height, buffer.data()))
      std::fprintf(stderr, "Failed to write to image file %s\n", output_path.string().c_str());
  } else {
    std::fprintf(stderr, "%s has an unrecognized extension\n", output_path.string().c_str());
  }
  if (configs.dump_raw &&
      !write_raw(*configs.dump_raw, resolution.width, resolution.height, [&](int which, float* dst) {
        if (ptc_download(path_tracer.handle(), which, dst, 0) < 0) throw std::runtime_error(ptc_last_error(path_tracer.handle()));
      }))
    std::fprintf(stderr, "Failed to write %s\n", configs.dump_raw->c_str());
  stopwatch.end_stage("Write image file");

  const ptc_stats st = path_tracer.stats();
  std::printf("Done path tracing %s!\n\n", scene_desc.filename.c_str());
  stopwatch.report();
  std::printf("rays: %llu  triangles: %u  bvh depth: %u\n", (unsigned long long)st.rays_total, st.triangle_count, st.bvh_max_depth);
  return 0;
} catch (const std::exception& e) {
  std::fprintf(stderr, "hip_pt fatal error: %s\n", e.what());
  return 1;
}
