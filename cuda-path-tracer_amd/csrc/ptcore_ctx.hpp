// ptcore_ctx.hpp -- private to libptcore.so: the context behind include/ptcore.h and the helpers its translation units share
// (ptcore.cpp: context, ptc_resize in stages -- refusals, the sizing plan, the old frame's release, a ptc_frame_state built beside the
// context, one assignment --, the parameter table, timed launches, views; ptcore_scene.cpp: scene upload in stages -- refusals and
// host preparation while the old scene stands, its release, device work, one assignment of ptc_scene_state; ptcore_trace.cpp: the launch plan of a
// batch of frames; ptcore_query.cpp: the ray queries outside the render loop; ptcore_bands.cpp: several GPUs; ptcore_display.cpp: the display transform; ptcore_checks.cpp:
// host-side checks of the schedule helpers).
#pragma once

#include "../../include/ptcore.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "pt_device.hpp"
#include "pt_host.hpp"
#include "pt_beam_rules.hpp"
#include "pt_feed_rules.hpp"
#include "pt_frame_rules.hpp"
#include "pt_env_light.hpp"

using namespace pt;

static_assert(sizeof(ptc_object) == sizeof(DObject), "ptc_object must match the device object");
static_assert(sizeof(ptc_material) == sizeof(DMaterial), "ptc_material must match the device material");
static_assert(sizeof(ptc_bvh_node) == 32, "BVH node is 32 bytes (bvh.hpp:30)");
static_assert(PTC_MAX_BOUNCES_CAP == kMaxBounces, "bounce cap mismatch");

// Everything of a context that describes the uploaded scene.  ptc_upload_scene (ptcore_scene.cpp) builds one of these beside the
// context and assigns it as a whole, after the last step that can fail; a value-initialised one is the state "no scene".  A
// field that depends on the scene belongs here.
struct ptc_scene_state {
  std::vector<void*> scene_allocs;  // every device array of the scene
  DScene scene{};
  bool has_scene = false;
  bool has_emitters = false;  // the scene's material table holds an emissive material (type 3): the shade kernels' kEmit instances
  uint32_t bvh_nodes = 0, bvh_depth = 0, triangles = 0;  // over all meshes (ptc_get_stats)
  ptc_upload_times upload_times{};
  std::vector<DMeshView> mesh_views;   // host copy of DScene::mesh_views: a traversal launch gets its object's mesh as DScene::cur
  std::vector<uint32_t> object_mesh;
  std::vector<uint32_t> mesh_nodes4;   // four-wide nodes of every mesh (k_beam's range check)
  // The closest-hit stage of the default variant, in object order: per mesh object a k_spheres launch for the run of
  // spheres in front of it ([pre_begin, pre_end), if it holds any) and a persistent traversal launch; the run that
  // ends the object list ([tail_begin, tail_end): everything, in a scene without a mesh) is tested by the kernel that ends the bounce (k_shade_fused; k_tail_count in the three-kernel form).
  struct TraceLaunch {
    uint32_t mesh, pre_begin, pre_end;
  };
  std::vector<TraceLaunch> launches;
  uint32_t tail_begin = 0, tail_end = 0;
  // per object: 0, or the class of a "simple" sphere object (sphere_ball_of) -- objects of one class have the same
  // matrix entries outside the translation columns; a run of one class (at most eight objects) takes sphere_run_lanes
  std::vector<uint32_t> sphere_class;
  uint64_t layout_counts[5] = {0, 0, 0, 0, 0};  // bytes of bvh4q, leaf_parent, tris, wide, bvh (ptc_download_layout)
  // direct-light queries (ptc_direct_light): the lamp table of the uploaded scene.  Kept out of DScene, which
  // every existing kernel takes by value.
  ptc_light_info light_info{};
  std::string light_error;               // not empty: an emissive sphere of the scene cannot be sampled (the query's refusal)
  uint32_t light_last = 0;               // last record with a weight > 0
  const float4* light_records = nullptr; // device: 4 float4 per record (ptc_light); null while there is nothing to sample
  const uint32_t* light_thresholds = nullptr;  // device: the records' selection thresholds, dense (the binary search)
  const float* light_material_pdf = nullptr;  // device: per material its records' inv_pdf, 0 for no lamp ("mis"); with the table
  // smooth shading (ptc_set_vertex_normals): the scene's vertex count, where each mesh's vertices start (device,
  // uploaded with the scene), and the normals -- a device array of the scene's pool, allocated by the first call that sets any;
  // normals_set: it holds the caller's normals now
  uint32_t vertex_count = 0;
  const uint32_t* mesh_first_vertex = nullptr;
  float* vertex_normals = nullptr;
  bool normals_set = false;
  // image textures (ptc_set_textures, ptc_set_texcoords): the scene's index and material counts and where each
  // mesh's corners start (device, uploaded with the scene); the coordinates, allocated by the first call that sets any; the texel
  // pool, the records, the per-material binding (replaced as a whole by every call that sets textures) and the two decode tables
  // (allocated by the first) -- all of the scene's pool
  uint32_t index_count = 0, material_count = 0;
  const uint32_t* mesh_first_index = nullptr;
  float* texcoords = nullptr;
  bool texcoords_set = false;
  uint32_t* tex_texels = nullptr;
  texmap::Record* tex_records = nullptr;
  int32_t* tex_material = nullptr;
  float* tex_table = nullptr;
  uint32_t texture_count = 0;
  uint64_t texel_count = 0;
  bool textures_set = false;
  // normal maps (ptc_set_normal_maps): per material -1 or a texture of the pool above (replaced as a whole by every
  // call that sets any; dropped by every ptc_set_textures, whose pool its indices name) and the decode table (allocated by the
  // first) -- of the scene's pool; nmap_bound: the materials with a map
  int32_t* nmap_material = nullptr;
  float* nmap_table = nullptr;
  uint32_t nmap_bound = 0;
  bool nmaps_set = false;
};

// the last epoch of a lap of look-back launches on a slot's tile descriptors (30 bits: pt_shade_tile.inc; ptcore_trace.cpp, next_epoch)
constexpr uint32_t kMaxEpoch = 0x3fffffffu;
// the counter block of the direct-lit megakernel (ptc_ctx::loop_stats)
constexpr size_t kLoopStatBytes = (size_t)kLightStatLines * kLoopStatWords * sizeof(unsigned long long);
constexpr size_t kVarianceStatBytes = kLoopStatBytes;  // k_variance_prefilter's counters, in lines as the albedo stage's: words 0, 1

// Everything of a context that a ptc_resize decides or that dies with it.  ptc_resize (ptcore.cpp) builds one of these beside the
// context and assigns it as a whole, after the last step that can fail; a value-initialised one is the state "no frame"
// (pix_capacity 0: "ptc_resize first" from every entry point); release_frame gives back what one owns.  A field that depends on
// the frame size belongs here.
struct ptc_frame_state {
  uint32_t width = 0, height = 0;
  uint32_t pix_begin = 0, pix_count = 0, pix_capacity = 0;
  DBand band{0, 0, 0, 1, 0};
  std::vector<void*> frame_allocs;  // every device array of the frame but the slots' spill areas and the band / gather buffers
  // Frames in flight: consecutive iterations are independent until they are folded into the framebuffer, and
  // the tail of every bounce is a handful of long rays (latency-bound), so iteration i runs on stream i % F
  // with its own path state and staging buffers; k_accumulate folds the staged samples in iteration order.
  struct FrameSlot {
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DPaths paths[2]{};
    DHits hits{};
    DHits hits_other{};             // "prefold": the second set of hit records (the shade kernel of bounce b writes bounce b + 1's while other
                                    // tiles still read bounce b's); `hits` is always the set the current bounce reads
    uint8_t* next_flags = nullptr;  // "prefold": per slot of the next bounce, does the ray go on the mesh launch's work list
    bool prefolded = false;         // ... the previous bounce's shade kernel has walked this bounce's leading sphere run (k_list_flags follows)
    uint32_t* chunk_counts = nullptr;   // "fused_shade" 0: k_tail_count -> k_scan -> k_shade
    uint32_t* chunk_offsets = nullptr;
    unsigned long long* tile_desc = nullptr;  // k_shade_fused: look-back descriptors, tile_stride per frame of the batch
    uint32_t tile_stride = 0;
    uint32_t shade_epoch = 0;           // look-back launches on these descriptors so far (1 .. kMaxEpoch, then round again; "debug_shade_epoch")
    float4* beam_entries = nullptr; // "beam": entry points of the batch's cameras (DBeam), capacity x tiles x 8 float4
    DBeam beam{};                   // ... as bounce 0's first traversal launch gets them (entries null: off for this batch)
    DCameras beam_cams{};           // the cameras (of the beams) the entries in beam_entries were computed for ...
    uint32_t beam_count = 0;        // ... how many, for which scene upload and mesh object: the next batch of this slot with
    uint64_t beam_scene = 0;        //     the same cameras (a viewer that accumulates, the benchmark) skips k_beam
    uint32_t beam_obj = 0;
    DPersist* persist = nullptr;    // "persist": the state of this slot's bounce-spanning launch (k_persist)
    uint32_t* slow_list = nullptr;  // slots of rays set aside for the exact redo at the end of a traversal launch
    uint32_t* slow_stack = nullptr; // that redo's traversal stack, [kStackDepth][kWave]
    uint8_t* octs = nullptr;        // "ray_sort": direction octant per slot of the rays of the next bounce
    uint32_t* order = nullptr;      // ... and the order in which the traversal lanes pick them up
    bool primary_finished = false;  // ... and finished the others itself: bounce 0's shade walks the list (launch_raygen)
    bool first_listed = false;      // ... k_raygen has listed the rays of bounce 0's first traversal launch (this batch)
    uint32_t* worklist = nullptr;   // "filter_rays": the rays of the next traversal launch that may hit one of its objects (k_spheres)
    uint2* spill = nullptr;         // traversal stack overflow area of this slot's launches (DScene::spill); grown by batch_begin, not in the pool
    size_t spill_elems = 0;
    DFrame stage{};
    DeviceCounters* counters = nullptr;  // one per frame of the batch
    hipEvent_t done = nullptr;  // after this slot's last accumulate
    uint32_t* live_host = nullptr;  // pinned: live[] of the slot's last batch (frame 0), copied back after `done`
    bool live_pending = false;      // ... and not yet looked at (launch sizing, see traverse_waves_for)
    int cur = 0;
    int work_slot = 0;
    int bounces_done = 0;
    DBatchInfo bi{};            // the batch being traced / traced last
    int capacity = 1;           // frames the slot's arrays hold
  };
  // Slots [0, big_slots) hold `batch` frames each; slots [big_slots, slots.size()) hold ONE frame: a batch of a
  // single iteration (a viewer that presents after every iteration, the stepwise calls) goes to one of those, so
  // that many such launches can be in flight on their own streams without the memory of full-size slots.
  std::vector<FrameSlot> slots;
  // Batches: up to `batch` consecutive iterations share the launches of a slot (DBatchInfo).  ptc_trace only
  // queues the iteration; the batch is enqueued when it is full or when anything else looks at the context.
  int batch = 1;          // allocated per big slot (frame_plan)
  bool staged = false;    // samples go through staging buffers and k_accumulate
  int big_slots = 0;
  uint32_t beam_tiles_x = 0, beam_tiles_y = 0;
  uint64_t batches_issued = 0, singles_issued = 0;  // round robin over the big and the single-frame slots
  int active_slot = -1;          // slot of the frame being built by ptc_trace_begin/bounce/end
  int last_slot = 0;             // slot of the most recent finished frame
  // live paths entering each bounce of one recent frame (what a frame of this scene / camera looks like): the host
  // never waits for them, they only size the traversal launches
  uint32_t est_live[2 * (kMaxBounces + 1)] = {};  // live[], then listed_now[] (DeviceCounters) of a recent batch's first frame
  bool est_valid = false;
  DFrame fb{};
  float4* den_a = nullptr;
  float4* den_b = nullptr;
  float4* den_pos = nullptr;     // per-pixel view-space hit position of the accumulated depth (denoiser)
  // "denoise_albedo" (DESIGN section 5r): the first-hit albedo plane and the irradiance plane, denoise_albedo_floats4 each
  // (pt_frame_rules.hpp); of frame_allocs, allocated by the first call that runs the stage at this frame size (albedo_planes)
  float4* den_albedo = nullptr;
  float4* den_irradiance = nullptr;
  // "denoise_variance" (DESIGN section 5s): the two variance planes, denoise_variance_floats each (pt_frame_rules.hpp); of
  // frame_allocs, allocated by the first call that runs the mode at this frame size (variance_planes)
  float* den_var_a = nullptr;
  float* den_var_b = nullptr;
  const float4* result = nullptr;
  float* pack_buf = nullptr;     // 3 floats / pixel staging for downloads
  uint32_t* rgba_buf = nullptr;  // staging for host presents
  DCamera cam{};                 // of the last traced frame, made for this width and height (ptc_denoise reuses it)
  bool have_cam = false;
  // several GPUs (ptc_band_*): this rank's exported band buffer (its handle dies with it: export again after a resize), and on
  // the root the peers' mapped buffers
  float* band_buf = nullptr;                // 3 floats per pixel of pix_capacity
  struct Peer {
    void* mapped = nullptr;                 // hipIpcOpenMemHandle of the peer process's band buffer
    bool opened = false;
    ptc_band_handle h{};
  };
  std::vector<Peer> peers;                  // by rank
  float* gather_frame = nullptr;            // root: the whole frame, 3 floats per pixel
  uint32_t* gather_rgba = nullptr;
  bool gather_timed = false;                // a gather of this frame has run (the events around it are the context's: gather_ev)
};

// What serves the frames and still stays here: the queue (pending, held) -- sync_frames traces what is queued, so it is empty
// whenever a frame state is released or assigned; active_slot indexes `slots` and est_live counts paths of a frame of this size,
// so those two are frame state -- and every event (order / main / xstream, turn_event, gather_ev, the timed launches'): created
// once, reused across resizes.  order_valid / main_valid are cleared by sync_frames.
struct ptc_ctx : ptc_scene_state, ptc_frame_state {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;

  // what the caller asked for (ptc_set_param, before ptc_resize): frame_plan turns it into ptc_frame_state's batch / slots
  int frames_in_flight = 64;
  bool frames_auto = true;  // not set by the caller: frame_plan caps it so that the in-flight state stays under kAutoFrameBytes
  int batch_frames = 32;
  struct Pending {
    DCamera cam;
    uint32_t iteration;
  };
  std::vector<Pending> pending;
  // "pair_batches" (round 5, measured: see DESIGN section 4d, the alternative that needs no hand-over inside a launch): a full
  // batch is HELD until the next one is full (or anything else looks at the context); the two are then enqueued bounce by
  // bounce on their two slots, and events make their traversal launches take turns -- A.T(0), B.T(0), A.T(1), ... -- so that the
  // kernels that end a bounce of one batch run beside the traversal launch of the other instead of beside nothing
  std::vector<Pending> held;
  int pair_batches = 0;
  hipEvent_t turn_event[2] = {nullptr, nullptr};  // recorded behind the traversal launches of a pair's two batches
  int turn_wait = -1;                             // which of them the next traversal launch of the pair waits for (-1: none)
  int turn_mine = -1;                             // which one the batch being enqueued records (-1: not a pair)
  hipEvent_t order_event = nullptr;  // last accumulate enqueued (accumulates run in iteration order)
  bool order_valid = false;
  hipEvent_t main_event = nullptr;   // last main-stream consumer that read the framebuffers asynchronously
  bool main_valid = false;
  DeviceCounters* misc_counters = nullptr;  // flags of kernels outside the frame loop (ptcore_query.cpp: exact_closest_hit)
  uint32_t slot_offset = 0;                 // "slot_offset" (multi-GPU: distinct random streams per rank)
  uint32_t* slot_offset_dev = nullptr;
  hipEvent_t xstream_event = nullptr;       // orders the stepwise calls between a frame's stream and ctx->stream
  hipEvent_t gather_ev[2] = {nullptr, nullptr};  // around the most recent gather launch (ptc_gather_last_us)

  int iteration = 0;
  int max_iterations = 1;
  int method = PTC_METHOD_STREAMING;
  int max_bounces = 50;
  ptc_denoiser_params den{10, 0.45f, 0.30f, 0.25f};
  uint64_t frames = 0;

  int trace_variant = 3;  // 3: persistent lanes over the four-wide collapse, conservative FMA slabs, exact check of the winner (default); 0: reference-order traversal; 1: culled near-first traversal with exact box decisions
  bool sphere_lanes = true;   // "sphere_lanes"
  bool sphere_fold = true;    // "sphere_fold"
  bool beam = true;           // "beam": primary rays start at their tile's entry points (k_beam)
  // "persist": bounces >= 1 of a batch and every shade pass as ONE launch (k_persist) when the launch plan is
  // one mesh object per bounce with nothing in front of it (ptcore_trace.cpp, persist_ok); 0: one launch per kernel and bounce
  int persist = 0;  // (off: measured 3 x slower than the per-bounce launches, DESIGN section 4d -- the service wavefronts are latency-bound)
  uint32_t persist_service_every = 5;  // "persist_service_every": one wavefront in this many shades, the others walk
  uint32_t persist_help_tiles = 8;     // "persist_help_tiles": tiles a walking wavefront without rays shades before it looks for rays again (0: it sleeps)
  uint32_t persist_min_frames = 2;     // "persist_min_frames": batches of fewer frames keep the per-bounce launches
  uint64_t scene_serial = 0;  // counts ptc_upload_scene calls (entry points computed for another scene are stale)
  uint32_t traverse_waves = 5120;
  uint32_t refill_lanes = 32;   // (20 until round 4: re-swept on its final code, profiles/r04_schedules.txt)
  uint32_t static_eighths = 4;  // (3 until round 4)
  bool merge_instances = true;  // "merge_instances": consecutive instances of one mesh walked by one launch (k_traverse4m)
  bool bvh_on_device = true;  // "bvh_build_on_device": the reference BVH of ptc_upload_scene from pt_bvh_gpu.hip
  bool layout_on_device = true;  // "layout_on_device": the traversal layouts derived from it, too
  uint32_t split_idle = 8;    // "split_idle"
  uint32_t min_waves = 1024;  // "min_waves": fewest persistent wavefronts of a traversal launch
  uint32_t small_waves = 3072;        // "small_waves": ... of a launch with fewer than small_rays_per_lane rays per lane of a full one
  uint32_t small_rays_per_lane = 4;   // "small_rays_per_lane" (8 until round 3: bounces 5 and 6 of a 20-frame batch -- 5 to 8 rays
                                      // per lane -- are 12-14 % faster on all 5120 wavefronts than on 3072)
  uint32_t run_waves = 3072;          // "run_waves" (round 5): most persistent wavefronts of a launch that walks a run of instances (k_traverse4m).
                                      // Config 2 -- 4.5 M listed rays per launch, two batches in flight -- 14.0 -> 14.8 Grays/s on 1536 ... 3584
                                      // wavefronts against 5120: the other batch's HBM-bound kernels get on the chip (profiles/r05_run_waves.txt)
  bool filter_rays = true;    // "filter_rays": a sphere run in front of a mesh launch also lists the rays that launch has to walk
  bool prefold = true;        // "prefold": the kernel that ends a bounce also walks the NEXT bounce's leading sphere run for its survivors (config 2's shape)
  bool fused_shade = true;    // "fused_shade": the end of a bounce in one pass (k_shade_fused); 0: k_tail_count -> k_scan -> k_shade
  int ray_sort = 0;           // "ray_sort": 1 = traversal lanes pick their rays up grouped by direction octant (bounces >= 1)
  int denoise_variant = 0;    // "denoise_variant": 0 = taps staged in LDS (default), 1 = taps through L1 / L2
  // "denoise_albedo" (DESIGN section 5r): ptc_denoise filters the colour divided by the first-hit albedo and multiplies it back.
  // albedo_stats: k_denoise_albedo's counter block on the device (kLoopStatBytes, the context's own; zeroed ahead of every launch, so
  // it holds the last launch's counts).  albedo_stage_ms: the stage's launches since ptc_restart (TimedLaunch::bounce == -2, counted
  // while their tag is albedo_epoch, which ptc_restart moves)
  bool denoise_albedo = false;
  unsigned long long* albedo_stats = nullptr;
  double albedo_stage_ms = 0.0;
  uint32_t albedo_epoch = 0;
  // "denoise_variance" (DESIGN section 5s): ptc_denoise estimates a per-pixel variance and lets it steer the passes' colour weight.
  // variance_sigma: ptc_set_denoise_variance.  variance_stats: k_variance_prefilter's counter block on the device (kLoopStatBytes; pixels, pixels on the
  // floor; zeroed ahead of every launch of the stage).  variance_stage_ms: the stage's launches since ptc_restart (TimedLaunch::bounce
  // == -3, counted while their tag is albedo_epoch, the one epoch ptc_restart moves)
  bool denoise_variance = false;
  float variance_sigma = 16.0f;
  unsigned long long* variance_stats = nullptr;
  double variance_stage_ms = 0.0;
  uint32_t lds_entries = kLds4;  // the kernels' LDS stack (pt_device.hpp); fewer only through "debug_lds_entries"
  int force_slow = 0;

  // measurement
  bool time_trace = false;
  bool count_tests = false;
  struct TimedLaunch {
    hipEvent_t start, stop;
    int bounce;
    uint32_t tag = 0;  // (bounce -2, -3) albedo_epoch when it was enqueued
  };
  std::vector<TimedLaunch> timed;        // recorded, not yet read
  std::vector<hipEvent_t> free_events;
  double trace_ms[kMaxBounces] = {};
  uint32_t trace_launches[kMaxBounces] = {};
  uint64_t intersect_redone = 0;         // rays ptc_intersect_rays redid exactly (reported as slow_rays[0])
  double denoise_ms = 0.0;               // A-Trous passes (TimedLaunch::bounce == -1)
  uint32_t denoise_passes = 0;
  uint32_t persist_launches = 0;         // batches traced through k_persist since ptc_reset_profile
  ptc_occlusion_stats occlusion{};       // ptc_occluded_rays since ptc_reset_profile

  ptc_direct_stats direct{};             // ptc_direct_light since ptc_reset_profile

  // The megakernel's options.  What they come to in a frame: mega_frame (ptcore_trace.cpp); which kernel that frame launches -- the one
  // named below only while no later option is on as well: the instance rule (pt_mega_rules.hpp).
  // "direct_light" (DESIGN section 5g): the megakernel draws a light sample at every diffuse hit (k_megakernel_direct)
  bool direct_light = false;
  // "roulette" (DESIGN section 5h): Russian roulette at every bounce >= this, the last bounce excepted; 0 = off
  int roulette = 0;
  // the thin lens (ptc_set_lens): radius 0 = the pinhole; every frame of a batch renders with one lens
  DLens lens{0.0f, 1.0f};
  // the environment (ptc_set_environment): the octahedral map with its apron on the device, or none (texels null:
  // the gradient, the instances launched as before); the context's own allocation -- it survives ptc_upload_scene and ptc_resize
  DEnv env{nullptr, 0u, 0u};
  // the environment as a light.  "environment_light": the megakernel draws an environment sample at every diffuse
  // hit (k_megakernel_env_light).  env_table: the alias table of env's map on the device, 16 n n bytes, the context's own allocation;
  // built by the first call that needs it (env_light_table), freed where the map is freed.  env_table_known: that call has been made
  // for this map -- a null table then means a map of weight 0
  bool environment_light = false;
  // "mis" (DESIGN section 5l): a frame that samples lamps or the environment combines each sample with the path's own continuation ray
  // by the balance heuristic (k_megakernel_mis); a frame that samples neither launches what it launched before
  bool mis = false;
  // "smooth_normals" (DESIGN section 5n): a frame of a scene with vertex normals shades triangle hits with the interpolated normal
  // (k_megakernel_smooth); without normals it launches what it launched before
  bool smooth_normals = false;
  // "textures" (DESIGN section 5o): a frame of a scene with textures and texture coordinates takes the colour of a bound diffuse or
  // metal triangle hit from its texture (k_megakernel_tex); without either it launches what it launched before
  bool textures = false;
  // "normal_maps" (DESIGN section 5q): a frame of a scene with textures, texture coordinates and a normal-map binding bends the normal
  // of a bound diffuse or metal triangle hit by its map (k_megakernel_nmap); without any of them it launches what it launched before
  bool normal_maps = false;
  const uint4* env_table = nullptr;
  bool env_table_known = false;
  ptc_environment_light_stats env_direct{};  // ptc_environment_light since ptc_reset_profile
  // device: kLightStatLines lines of kLoopStatWords words (0 .. 2 the lamps': diffuse hits, shadow rays, unoccluded; 3 .. 5 the environment's;
  // 6, 7 "mis": weighted emitter hits, weighted misses; 8 .. 11 "smooth_normals": shading normals, fall-backs, absorbed, culled;
  // 12, 13 "textures": lookups, fall-backs; 14, 15 "normal_maps": bent normals, fall-backs)
  unsigned long long* loop_stats = nullptr;
  bool loop_stats_clear = true;              // ptc_restart has run since the last direct-lit launch: that launch's stream zeroes the block first
  // the display transform (ptc_set_display; ptcore_display.cpp).  The default is the reference display: the presents
  // launch k_preview as before and nothing below is touched.  meter_dev / exposure_dev: one allocation of the context's own, made by the
  // first present that needs it; the accumulation words are zero between calls.  shown: the last present's DExposure, for
  // ptc_get_exposure_info
  ptc_display_params display{PTC_CURVE_CLAMP, 0, 1.0f, 0.18f, 4.0f, 50u, 950u};
  DMeter* meter_dev = nullptr;
  DExposure* exposure_dev = nullptr;
  DExposure shown{};
  bool shown_known = false;
};

namespace ptcd {

extern thread_local std::string g_create_error;
void request_hw_queues();
int fail(ptc_ctx* ctx, int code, const std::string& msg);

#define HIP_TRY(ctx, expr)                                                                      \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return fail(ctx, e_ == hipErrorOutOfMemory ? PTC_ERR_OOM : PTC_ERR_HIP,                   \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                           \
  } while (0)

int check_last(ptc_ctx* ctx, const char* what);
// HIP events around one launch of a timed kernel, on the stream it runs on (ptcore.cpp; a closest-hit launch of `bounce`, an
// A-Trous pass with bounce -1, a launch of the "denoise_albedo" stage with bounce -2, of the "denoise_variance" estimate stage with -3).  Nothing while ctx->time_trace is off.
int timed_begin(ptc_ctx* ctx, hipStream_t stream, int bounce, ptc_ctx::TimedLaunch* tl);
int timed_end(ptc_ctx* ctx, hipStream_t stream, const ptc_ctx::TimedLaunch& tl);
int bind_device(ptc_ctx* ctx);
void free_pool(std::vector<void*>& pool);
DCamera make_camera(const ptc_camera& c, uint32_t w, uint32_t h);
int flush_pending(ptc_ctx* ctx, bool from_trace = false);  // enqueue the iterations ptc_trace has queued (ptcore_trace.cpp)
uint32_t fold_run_of(const ptc_ctx* ctx, uint32_t begin, uint32_t end);  // may k_spheres take sphere_fold for this run? (ptcore_trace.cpp)
uint32_t lanes_run_of(const ptc_ctx* ctx, uint32_t begin, uint32_t end);  // ... the per-lane form, sphere_run_lanes? (ptcore_trace.cpp)
int sync_frames(ptc_ctx* ctx);
// "roulette" (DESIGN section 5h): does any bounce of a frame play?  (ptcore_trace.cpp: the one statement of it)
bool roulette_frame(int roulette, int max_bounces);
// The alias table of the context's environment (ptcore.cpp), built and uploaded if this map has none yet.  After
// PTC_OK ctx->env_table is the table, or null for a map of weight 0.  PTC_ERR_OOM: the allocation failed; the environment stays.
int env_light_table(ptc_ctx* ctx);
// gives back everything a frame state owns and leaves it "no frame" (ptcore.cpp); its streams must be idle (sync_frames)
void release_frame(ptc_frame_state& f);
int frame_ready(ptc_ctx* ctx);
// The views (ptcore.cpp).  view_ready: the opening their entry points share -- NULL is PTC_ERR_INVALID, "ptc_resize first", the device.
// buffer_view: the one reading of a ptc_buffer ("unknown buffer"); display_view: of a ptc_display ("unknown display type").
struct BufferView { const float4* src; int sel; uint32_t floats_per_pixel; };  // framebuffer, launch_pack's selector, floats of a packed pixel
struct DisplayView { int which, mode; };                                       // the ptc_buffer shown, launch_preview's mode
int view_ready(ptc_ctx* ctx, const void* arg);
int buffer_view(ptc_ctx* ctx, int which, BufferView* out);
int display_view(ptc_ctx* ctx, int display_type, bool gathered, DisplayView* out);
// The display transform (ptcore_display.cpp).  reference_display: the display under which a present launches
// k_preview as it always did.  show_display: meter (under metering 1), level and tone-map n pixels of src4 (a float4 each) or src3
// (three floats each) on ctx->stream, into rgba and / or mapped (device; either may be null); *shown gets the DExposure of this call
// once the stream has been synchronised, which is the caller's to do.
bool reference_display(const ptc_display_params& d);
int show_display(ptc_ctx* ctx, const float4* src4, const float* src3, uint32_t n, uint32_t* rgba, float* mapped, DExposure* shown);
// The lamp table of a validated scene (ptcore_scene.cpp; include/ptcore.h: ptc_light).  *last = last record with a weight > 0.
// thresholds (may be null): per record what light_pick searches (pt_light_sample.hpp), empty for a table of weight 0.
// Returns PTC_OK, or PTC_ERR_INVALID with `err` naming the emissive sphere whose matrix is no similarity.
int build_light_table(const ptc_scene_desc* s, std::vector<ptc_light>& out, ptc_light_info* info, uint32_t* last, std::string* err,
                      std::vector<uint32_t>* thresholds);
// ... of a scene as the caller hands it over: validate_scene's and build_light_table's refusals, with their message (ptc_last_error(NULL))
// What ptc_set_textures and ptc_check_texture_lookup refuse in one texture (ptcore_scene.cpp): the rest of the sentence "texture i
// ...", or "" for a texture they take
std::string texture_refusal(const ptc_texture_desc& t);
int checked_light_table(const ptc_scene_desc* s, std::vector<ptc_light>& out, ptc_light_info* info, uint32_t* last,
                        std::vector<uint32_t>* thresholds);

// What a traversal launch over n rays needs besides its rays, outside a frame slot (ptcore_query.cpp).  The queries allocate it per
// call (alloc_walk_scratch, into the call's pool); a bounce loop would fill it with its slot's buffers instead.
struct WalkScratch {
  uint32_t* slow_list = nullptr;       // n entries
  uint32_t* slow_stack = nullptr;      // kStackDepth * kWave
  uint2* spill = nullptr;              // scene.spill_cap * scene.spill_stride
  DeviceCounters* counters = nullptr;  // one block; its slow_rays[0] and flags are the launches' results
  uint32_t* chunk_counts = nullptr;    // n / kChunk + 1 entries, for launch_tail_count: the closest-hit query alone asks for it
};
int alloc_walk_scratch(ptc_ctx* ctx, std::vector<void*>& pool, uint32_t n, bool want_chunks, WalkScratch* scr);
int occlude_on_device(ptc_ctx* ctx, hipStream_t stream, const float4* rays_o4, const float4* rays_d4, uint32_t n, uint8_t* flags,
                      const WalkScratch& scr, uint32_t* launches);

template <typename T>
int dev_alloc(ptc_ctx* ctx, std::vector<void*>& pool, T** out, size_t count)
{
  void* p = nullptr;
  const size_t bytes = std::max<size_t>(count * sizeof(T), 256);
  HIP_TRY(ctx, hipMalloc(&p, bytes));
  pool.push_back(p);
  *out = static_cast<T*>(p);
  return PTC_OK;
}

template <typename T>
int upload(ptc_ctx* ctx, std::vector<void*>& pool, const T** out, const T* host, size_t count)
{
  T* d = nullptr;
  int rc = dev_alloc(ctx, pool, &d, count);
  if (rc) return rc;
  if (count) HIP_TRY(ctx, hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
  *out = d;
  return PTC_OK;
}

}  // namespace ptcd

