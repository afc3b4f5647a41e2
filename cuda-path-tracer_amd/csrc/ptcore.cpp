// ptcore.cpp -- the C ABI of libptcore.so (include/ptcore.h): context, buffers, frame loop.
//
// One ptc_ctx owns what the reference's PathTracer owns (path_tracer.hpp:68-84): the device scene, the
// path state, the hit records, the accumulated framebuffers, the two denoise ping-pong buffers and the
// iteration counter.  Differences that matter for speed, not results:
//   - no per-bounce host synchronisation: live-path counts stay in a device counter block and the
//     kernels of bounce b read live[b] themselves (the reference reads the Thrust partition result
//     back every bounce, path_tracer.cu:457);
//   - path state is ping-ponged between two buffers by the fused shade+compaction kernel instead of
//     being partitioned in place through a Thrust temporary.
//
// This unit: context; ptc_resize in stages (refusals, frame_plan, release of the old frame, a ptc_frame_state built beside the
// context, ONE assignment) and release_frame, the one release path; parameters; denoise; the views (buffer_view / display_view);
// statistics (each_counter_block).  Scene upload: ptcore_scene.cpp; the launch plan of a batch: ptcore_trace.cpp; the ray queries: ptcore_query.cpp; several GPUs: ptcore_bands.cpp;
// host-side checks: ptcore_checks.cpp.
#include "ptcore_ctx.hpp"

using namespace pt;
using namespace ptcd;

namespace ptcd {

thread_local std::string g_create_error;

// The frames in flight run on separate HIP streams, and streams only overlap when they sit on different
// hardware queues; the runtime's default is 4 queues per process.  Ask for more before this library's first HIP
// call (no effect if the application has set the variable or has already initialised HIP itself: such an
// application exports GPU_MAX_HW_QUEUES on its own, see ptcore.h).
void request_hw_queues()
{
  static const int once = setenv("GPU_MAX_HW_QUEUES", "24", 0);
  (void)once;
}

int fail(ptc_ctx* ctx, int code, const std::string& msg)
{
  if (ctx) ctx->err = msg;
  else g_create_error = msg;
  return code;
}

int check_last(ptc_ctx* ctx, const char* what)
{
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ctx, PTC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  return PTC_OK;
}

// HIP events around one launch of a timed kernel, on the stream it runs on.  The events come from free_events, where drain_timed
// puts them back when it has read the pair that timed_end left in ctx->timed.
int timed_begin(ptc_ctx* ctx, hipStream_t stream, int bounce, ptc_ctx::TimedLaunch* tl)
{
  *tl = ptc_ctx::TimedLaunch{nullptr, nullptr, bounce};
  if (!ctx->time_trace) return PTC_OK;
  for (hipEvent_t* e : {&tl->start, &tl->stop}) {
    if (!ctx->free_events.empty()) {
      *e = ctx->free_events.back();
      ctx->free_events.pop_back();
    } else {
      HIP_TRY(ctx, hipEventCreate(e));
    }
  }
  HIP_TRY(ctx, hipEventRecord(tl->start, stream));
  return PTC_OK;
}

int timed_end(ptc_ctx* ctx, hipStream_t stream, const ptc_ctx::TimedLaunch& tl)
{
  if (!ctx->time_trace) return PTC_OK;
  HIP_TRY(ctx, hipEventRecord(tl.stop, stream));
  ctx->timed.push_back(tl);
  return PTC_OK;
}

int bind_device(ptc_ctx* ctx)
{
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return PTC_OK;
}

void free_pool(std::vector<void*>& pool)
{
  for (void* p : pool) (void)hipFree(p);
  pool.clear();
}

// Camera::to_gpu_camera (camera.cpp:5-13) + the frame-invariant part of generate_ray (ray_gen.cu:37-47)
DCamera make_camera(const ptc_camera& c, uint32_t w, uint32_t h)
{
  DCamera d;
  d.cam = camera_matrix(c.position, c.rotation_wxyz);
  const f4 o = mul(d.cam, 0.0f, 0.0f, 0.0f, 1.0f);
  d.origin = mk3(o.x, o.y, o.z);
  const float aspect = (float)w / (float)h;
  d.vh = 2.0f * tanf(c.vfov / 2);
  d.vw = aspect * d.vh;
  // lower_left_corner = origin - horizontal/2 - vertical/2 - (0,0,focal)
  d.llx = ((0.0f - d.vw / 2.f) - 0.0f / 2.f) - 0.0f;
  d.lly = ((0.0f - 0.0f / 2.f) - d.vh / 2.f) - 0.0f;
  d.width = w;
  d.height = h;
  return d;
}

// wait (host-side) until every frame in flight has been folded into the framebuffers
int sync_frames(ptc_ctx* ctx)
{
  if (int rc = flush_pending(ctx)) return rc;
  for (auto& sl : ctx->slots)
    if (sl.stream) HIP_TRY(ctx, hipStreamSynchronize(sl.stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->order_valid = false;
  ctx->main_valid = false;
  return PTC_OK;
}

// The one release path of a frame state (ptc_resize: the old frame, and a new one that did not get to the commit; ptc_destroy).
// Events that outlive a frame -- gather_ev, the timed launches' -- are the context's and stay.
void release_frame(ptc_frame_state& f)
{
  for (auto& sl : f.slots) {
    if (sl.own_stream && sl.stream) (void)hipStreamDestroy(sl.stream);
    if (sl.done) (void)hipEventDestroy(sl.done);
    if (sl.live_host) (void)hipHostFree(sl.live_host);
    if (sl.spill) (void)hipFree(sl.spill);
  }
  free_pool(f.frame_allocs);
  for (auto& peer : f.peers)
    if (peer.opened && peer.mapped) (void)hipIpcCloseMemHandle(peer.mapped);
  for (void* q : {(void*)f.band_buf, (void*)f.gather_frame, (void*)f.gather_rgba})
    if (q) (void)hipFree(q);
  f = ptc_frame_state{};
}

int frame_ready(ptc_ctx* ctx)
{
  if (!ctx) return PTC_ERR_INVALID;
  if (!ctx->has_scene) return fail(ctx, PTC_ERR_NO_SCENE, "no scene uploaded");
  if (!ctx->pix_capacity) return fail(ctx, PTC_ERR_INVALID, "ptc_resize first");
  return bind_device(ctx);
}

int view_ready(ptc_ctx* ctx, const void* arg)
{
  if (!ctx || !arg) return PTC_ERR_INVALID;
  if (!ctx->pix_capacity) return fail(ctx, PTC_ERR_INVALID, "ptc_resize first");
  return bind_device(ctx);
}

// the two tables of the views, by ptc_buffer (colour, normal, depth, final) and by ptc_display (final, colour, normal, depth)
static_assert(PTC_BUF_COLOR == 0 && PTC_BUF_FINAL == 3 && PTC_DISPLAY_FINAL == 0 && PTC_DISPLAY_DEPTH == 3, "the view tables' order");
int buffer_view(ptc_ctx* ctx, int which, BufferView* out)
{
  if (which < PTC_BUF_COLOR || which > PTC_BUF_FINAL) return fail(ctx, PTC_ERR_INVALID, "unknown buffer");
  const BufferView views[] = {{ctx->fb.color4, 0, 3u}, {ctx->fb.nd4, 0, 3u}, {ctx->fb.nd4, 1, 1u}, {ctx->result, 0, 3u}};
  *out = views[which];
  return PTC_OK;
}

int display_view(ptc_ctx* ctx, int display_type, bool gathered, DisplayView* out)
{
  if (display_type < PTC_DISPLAY_FINAL || display_type > PTC_DISPLAY_DEPTH) return fail(ctx, PTC_ERR_INVALID, "unknown display type");
  // a gathered FINAL shows the accumulated colour: a denoised buffer exists only for a context that owns the whole frame
  const DisplayView views[] = {{gathered ? PTC_BUF_COLOR : PTC_BUF_FINAL, 0}, {PTC_BUF_COLOR, 0}, {PTC_BUF_NORMAL, 1}, {PTC_BUF_DEPTH, 2}};
  *out = views[display_type];
  return PTC_OK;
}

}  // namespace ptcd

namespace {

// ptc_set_param (documented in include/ptcore.h): one row per parameter that stores a checked value -- the inclusive range and what
// follows the name in the refusal of a value outside it, whether it must be set before ptc_resize (it sizes the frame slots) or
// before ptc_upload_scene (it sizes the scene), and where the value goes.  The range is checked before the gate.
enum ParamGate { kAnyTime, kBeforeResize, kBeforeUpload };
struct ParamRow {
  const char* name;
  int lo, hi;
  const char* complaint;
  ParamGate gate;
  void (*store)(ptc_ctx* c, int v);
};
#define PT_STR2(x) #x
#define PT_STR(x) PT_STR2(x)
constexpr const char* k01 = " must be 0 or 1";
constexpr const char* kRange = " out of range";
const ParamRow kParams[] = {
    {"batch_frames", 1, kMaxBatch, " must be in [1,32]", kBeforeResize, [](ptc_ctx* c, int v) { c->batch_frames = v; }},
    {"traverse_waves", 8, 65536, kRange, kBeforeUpload, [](ptc_ctx* c, int v) { c->traverse_waves = (uint32_t)v; }},
    {"debug_lds_entries", 1, kLds4, " must be in [1," PT_STR(PT_T4_LDS) "]", kBeforeUpload,
     [](ptc_ctx* c, int v) { c->lds_entries = (uint32_t)v; }},
    {"layout_on_device", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->layout_on_device = v != 0; }},
    {"filter_rays", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->filter_rays = v != 0; }},
    {"fused_shade", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->fused_shade = v != 0; }},
    {"merge_instances", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->merge_instances = v != 0; }},
    {"bvh_build_on_device", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->bvh_on_device = v != 0; }},
    {"static_eighths", 0, 8, " must be in [0,8]", kAnyTime,
     [](ptc_ctx* c, int v) { c->scene.static_eighths = c->static_eighths = (uint32_t)v; }},
    {"small_waves", 8, 65536, kRange, kAnyTime, [](ptc_ctx* c, int v) { c->small_waves = (uint32_t)v; }},
    {"small_rays_per_lane", 0, 1024, kRange, kAnyTime, [](ptc_ctx* c, int v) { c->small_rays_per_lane = (uint32_t)v; }},
    {"run_waves", 8, 65536, kRange, kAnyTime, [](ptc_ctx* c, int v) { c->run_waves = (uint32_t)v; }},
    {"min_waves", 8, 65536, kRange, kAnyTime, [](ptc_ctx* c, int v) { c->min_waves = (uint32_t)v; }},
    {"beam", 0, 1, k01, kBeforeResize, [](ptc_ctx* c, int v) { c->beam = v != 0; }},
    {"persist", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->persist = v; }},
    {"persist_service_every", 2, 64, " must be in [2, 64]", kAnyTime,
     [](ptc_ctx* c, int v) { c->persist_service_every = (uint32_t)v; }},
    {"prefold", 0, 1, k01, kBeforeResize, [](ptc_ctx* c, int v) { c->prefold = v != 0; }},
    {"pair_batches", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->pair_batches = v; }},
    {"persist_help_tiles", 0, 4096, " must be in [0, 4096]", kAnyTime, [](ptc_ctx* c, int v) { c->persist_help_tiles = (uint32_t)v; }},
    {"persist_min_frames", 1, kMaxBatch, " must be in [1, 32]", kAnyTime, [](ptc_ctx* c, int v) { c->persist_min_frames = (uint32_t)v; }},
    {"sphere_fold", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->sphere_fold = v != 0; }},
    {"sphere_lanes", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->sphere_lanes = v != 0; }},
    {"split_idle", 0, 64, " must be in [0,64]", kAnyTime, [](ptc_ctx* c, int v) { c->scene.split_idle = c->split_idle = (uint32_t)v; }},
    {"refill_lanes", 1, 64, " must be in [1,64]", kAnyTime,
     [](ptc_ctx* c, int v) { c->scene.refill_lanes = c->refill_lanes = (uint32_t)v; }},
    {"ray_sort", 0, 1, k01, kBeforeResize, [](ptc_ctx* c, int v) { c->ray_sort = v; }},
    {"direct_light", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->direct_light = v != 0; }},
    {"environment_light", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->environment_light = v != 0; }},
    {"mis", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->mis = v != 0; }},
    {"smooth_normals", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->smooth_normals = v != 0; }},
    {"textures", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->textures = v != 0; }},
    {"normal_maps", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->normal_maps = v != 0; }},
    {"roulette", 0, 64, " must be in [0,64]", kAnyTime, [](ptc_ctx* c, int v) { c->roulette = v; }},
    {"denoise_variant", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->denoise_variant = v; }},
    {"denoise_albedo", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->denoise_albedo = v != 0; }},
    {"denoise_variance", 0, 1, k01, kAnyTime, [](ptc_ctx* c, int v) { c->denoise_variance = v != 0; }},
    {"frames_in_flight", 1, 256, " must be in [1,256]", kBeforeResize, [](ptc_ctx* c, int v) { c->frames_in_flight = v; }},
};
#undef PT_STR
#undef PT_STR2
static_assert(kMaxBatch == 32, "the range messages of batch_frames and persist_min_frames spell the bound out");

// "slot_offset", the one parameter that lives on the device
int set_slot_offset(ptc_ctx* ctx, int value)
{
  if (value < 0) return fail(ctx, PTC_ERR_INVALID, "slot_offset must not be negative");
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;  // frames in flight read the offset when they execute
  ctx->slot_offset = (uint32_t)value;
  HIP_TRY(ctx, hipMemcpy(ctx->slot_offset_dev, &ctx->slot_offset, sizeof(uint32_t), hipMemcpyHostToDevice));
  return PTC_OK;
}

// "debug_shade_epoch": every slot as if it had seen `value` look-back launches and none of them had left a descriptor
int set_shade_epoch(ptc_ctx* ctx, int value)
{
  if (value < 0 || (uint32_t)value > kMaxEpoch) return fail(ctx, PTC_ERR_INVALID, "debug_shade_epoch must be in [0,1073741823]");
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;  // frames in flight carry the epochs they were enqueued with
  for (auto& sl : ctx->slots) {
    // (a descriptor of an earlier launch may carry an epoch above `value`, which a launch to come would take again)
    HIP_TRY(ctx, hipMemset(sl.tile_desc, 0, sizeof(unsigned long long) * (size_t)sl.capacity * sl.tile_stride));
    sl.shade_epoch = (uint32_t)value;
  }
  return PTC_OK;
}
static_assert(kMaxEpoch == 1073741823u, "the range message of debug_shade_epoch spells the bound out");

// ---- the counter blocks: one DeviceCounters per slot and frame of its batch; their head is everything but the fetch cursors
constexpr size_t kCountersHead = offsetof(DeviceCounters, work);
// visit(slot, frame of the slot's batch, the block on the device) for every block, in slot order; stops at the first failure
template <typename Visit>
int each_counter_block(ptc_ctx* ctx, Visit visit)
{
  for (size_t f = 0; f < ctx->slots.size(); ++f)
    for (int k = 0; k < ctx->slots[f].capacity; ++k)
      if (int rc = visit(f, k, ctx->slots[f].counters + k)) return rc;
  return PTC_OK;
}

// ... with the block's head on the host: one copy per block
template <typename Visit>
int each_counter_head(ptc_ctx* ctx, Visit visit)
{
  std::vector<char> buf(sizeof(DeviceCounters));
  return each_counter_block(ctx, [&](size_t f, int k, const DeviceCounters* dev) -> int {
    HIP_TRY(ctx, hipMemcpy(buf.data(), dev, kCountersHead, hipMemcpyDeviceToHost));
    visit(f, k, *reinterpret_cast<const DeviceCounters*>(buf.data()));
    return PTC_OK;
  });
}

// ---- ptc_resize: a frame state in the making, assigned to the context as a whole; released with this struct if it never gets there
struct NewFrame : ptc_frame_state {
  ~NewFrame() { release_frame(*this); }
};

// One slot of `capacity` frames of P pixels: its stream and event, path state, hit records, lists, counters and staging.
int build_slot(ptc_ctx* ctx, NewFrame& n, ptc_ctx::FrameSlot& sl, int capacity, size_t P)
{
  auto& pool = n.frame_allocs;
  const size_t chunks = (P + kChunk - 1) / kChunk;
  sl.capacity = capacity;
  sl.stream = ctx->stream;  // one frame in flight: trace on the context's stream (ptc_set_stream keeps it so)
  if (n.staged) {
    HIP_TRY(ctx, hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
    sl.own_stream = true;
  }
  HIP_TRY(ctx, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
  HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void**>(&sl.live_host), sizeof(uint32_t) * 2 * (kMaxBounces + 1), hipHostMallocDefault));
  const size_t BP = (size_t)capacity * P;  // frame f of the batch at element offset f * P (DBatchInfo::stride)
  for (int k = 0; k < 2; ++k) {
    if (int rc = dev_alloc(ctx, pool, &sl.paths[k].o4, BP)) return rc;
    if (int rc = dev_alloc(ctx, pool, &sl.paths[k].d4, BP)) return rc;
    if (int rc = dev_alloc(ctx, pool, &sl.paths[k].t2, BP)) return rc;
  }
  if (int rc = dev_alloc(ctx, pool, &sl.hits.tp, BP)) return rc;
  if (int rc = dev_alloc(ctx, pool, &sl.hits.nm, BP)) return rc;
  if (ctx->prefold) {
    if (int rc = dev_alloc(ctx, pool, &sl.hits_other.tp, BP)) return rc;
    if (int rc = dev_alloc(ctx, pool, &sl.hits_other.nm, BP)) return rc;
    if (int rc = dev_alloc(ctx, pool, &sl.next_flags, BP)) return rc;
  }
  if (int rc = dev_alloc(ctx, pool, &sl.chunk_counts, (size_t)capacity * chunks)) return rc;
  if (int rc = dev_alloc(ctx, pool, &sl.chunk_offsets, (size_t)capacity * chunks)) return rc;
  // (tile descriptors: k_shade_fused's 512-slot tiles, or the persistent launch's 128-slot ones)
  sl.tile_stride = std::max(shade_tiles_per_frame((uint32_t)P), persist_tiles_per_frame((uint32_t)P));
  if (int rc = dev_alloc(ctx, pool, &sl.tile_desc, (size_t)capacity * sl.tile_stride)) return rc;
  HIP_TRY(ctx, hipMemsetAsync(sl.tile_desc, 0, sizeof(unsigned long long) * (size_t)capacity * sl.tile_stride, ctx->stream));
  if (int rc = dev_alloc(ctx, pool, &sl.slow_list, BP)) return rc;
  if (n.staged) {
    if (int rc = dev_alloc(ctx, pool, &sl.persist, 1)) return rc;
    HIP_TRY(ctx, hipMemsetAsync(sl.persist, 0, sizeof(DPersist), ctx->stream));
  }
  if (int rc = dev_alloc(ctx, pool, &sl.slow_stack, (size_t)kStackDepth * kWave)) return rc;
  if (ctx->beam)
    if (int rc = dev_alloc(ctx, pool, &sl.beam_entries, (size_t)capacity * n.beam_tiles_x * n.beam_tiles_y * 2u * kBeamEntries)) return rc;
  if (int rc = dev_alloc(ctx, pool, &sl.worklist, BP)) return rc;
  if (ctx->ray_sort) {
    if (int rc = dev_alloc(ctx, pool, &sl.octs, BP)) return rc;
    if (int rc = dev_alloc(ctx, pool, &sl.order, BP)) return rc;
  }
  if (int rc = dev_alloc(ctx, pool, &sl.counters, (size_t)capacity)) return rc;
  HIP_TRY(ctx, hipMemsetAsync(sl.counters, 0, sizeof(DeviceCounters) * (size_t)capacity, ctx->stream));
  sl.bi.stride = (uint32_t)P;
  sl.bi.chunk_stride = (uint32_t)chunks;
  sl.bi.count = 1u;
  sl.stage = n.fb;  // one frame in flight: shade accumulates straight into the framebuffers
  if (n.staged) {
    if (int rc = dev_alloc(ctx, pool, &sl.stage.color4, BP)) return rc;
    if (int rc = dev_alloc(ctx, pool, &sl.stage.nd4, BP)) return rc;
  }
  return PTC_OK;
}

// The frame state of a width x height frame under `plan`, into n: nothing of the context is assigned here.
int build_frame(ptc_ctx* ctx, uint32_t width, uint32_t height, const ptc_frame_plan& plan, NewFrame& n)
{
  const size_t P = (size_t)width * height;
  auto& pool = n.frame_allocs;
  n.batch = plan.batch;
  n.staged = plan.staged != 0;
  n.big_slots = plan.big_slots;
  n.beam_tiles_x = (width + kBeamTile - 1u) / kBeamTile;  // ("beam": the slots' entry points)
  n.beam_tiles_y = (height + kBeamTile - 1u) / kBeamTile;
  if (int rc = dev_alloc(ctx, pool, &n.fb.color4, P)) return rc;
  if (int rc = dev_alloc(ctx, pool, &n.fb.nd4, P)) return rc;
  n.slots.resize((size_t)(plan.big_slots + plan.single_slots));
  for (int f = 0; f < (int)n.slots.size(); ++f)
    if (int rc = build_slot(ctx, n, n.slots[(size_t)f], f < plan.big_slots ? plan.batch : 1, P)) return rc;
  for (float4** q : {&n.den_a, &n.den_b, &n.den_pos})
    if (int rc = dev_alloc(ctx, pool, q, P)) return rc;
  if (int rc = dev_alloc(ctx, pool, &n.pack_buf, P * 3u)) return rc;
  if (int rc = dev_alloc(ctx, pool, &n.rgba_buf, P)) return rc;
  for (float4* q : {n.fb.color4, n.fb.nd4, n.den_a, n.den_b}) HIP_TRY(ctx, hipMemsetAsync(q, 0, P * sizeof(float4), ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  n.width = width;
  n.height = height;
  n.band = DBand{0u, width, 0u, 1u, 0u};
  n.pix_count = n.pix_capacity = (uint32_t)P;
  n.result = n.fb.color4;
  return PTC_OK;
}

}  // namespace

extern "C" {

int ptc_abi_version(void) { return PTC_ABI_VERSION; }

int ptc_device_count(int* count)
{
  if (!count) return PTC_ERR_INVALID;
  request_hw_queues();
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    (void)hipGetLastError();
    return fail(nullptr, PTC_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *count = n;
  return PTC_OK;
}

const char* ptc_last_error(const ptc_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int ptc_create(const ptc_config* config, ptc_ctx** out)
{
  if (!out) return fail(nullptr, PTC_ERR_INVALID, "out is NULL");
  *out = nullptr;
  request_hw_queues();
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    return fail(nullptr, PTC_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
  }
  const int device = config ? config->device : 0;
  if (device < 0 || device >= n) return fail(nullptr, PTC_ERR_NO_DEVICE, "device ordinal out of range");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(nullptr, PTC_ERR_HIP, "hipGetDeviceProperties failed");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, PTC_ERR_NO_DEVICE, std::string("kernels are built for gfx950 only; device is ") + prop.gcnArchName);

  ptc_ctx* ctx = new (std::nothrow) ptc_ctx();
  if (!ctx) return fail(nullptr, PTC_ERR_OOM, "out of host memory");
  ctx->device = device;
  if (config) {
    if (config->max_bounces > 0) ctx->max_bounces = std::min(config->max_bounces, (int)kMaxBounces);
    if (config->method == PTC_METHOD_MEGAKERNEL) ctx->method = PTC_METHOD_MEGAKERNEL;
  }
  auto bail = [&](int rc) {
    g_create_error = ctx->err;
    ptc_destroy(ctx);
    return rc;
  };
  if (hipSetDevice(device) != hipSuccess) return bail(fail(ctx, PTC_ERR_HIP, "hipSetDevice failed"));
  if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess)
    return bail(fail(ctx, PTC_ERR_HIP, "hipStreamCreate failed"));
  ctx->stream = ctx->own_stream;
  void* p = nullptr;
  if (hipMalloc(&p, sizeof(DeviceCounters)) != hipSuccess) return bail(fail(ctx, PTC_ERR_OOM, "hipMalloc(counters) failed"));
  ctx->misc_counters = static_cast<DeviceCounters*>(p);
  if (hipMemset(ctx->misc_counters, 0, sizeof(DeviceCounters)) != hipSuccess) return bail(fail(ctx, PTC_ERR_HIP, "hipMemset failed"));
  if (hipEventCreateWithFlags(&ctx->order_event, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->main_event, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->xstream_event, hipEventDisableTiming) != hipSuccess)
    return bail(fail(ctx, PTC_ERR_HIP, "hipEventCreate failed"));
  if (hipMalloc(&p, 256) != hipSuccess) return bail(fail(ctx, PTC_ERR_OOM, "hipMalloc(slot offset) failed"));
  ctx->slot_offset_dev = static_cast<uint32_t*>(p);
  if (hipMemset(ctx->slot_offset_dev, 0, 256) != hipSuccess) return bail(fail(ctx, PTC_ERR_HIP, "hipMemset failed"));
  if (hipMalloc(&p, kLoopStatBytes) != hipSuccess) return bail(fail(ctx, PTC_ERR_OOM, "hipMalloc(direct-light loop counters) failed"));
  ctx->loop_stats = static_cast<unsigned long long*>(p);
  if (hipMalloc(&p, kLoopStatBytes) != hipSuccess) return bail(fail(ctx, PTC_ERR_OOM, "hipMalloc(denoise albedo counters) failed"));
  ctx->albedo_stats = static_cast<unsigned long long*>(p);
  if (hipMemset(ctx->albedo_stats, 0, kLoopStatBytes) != hipSuccess) return bail(fail(ctx, PTC_ERR_HIP, "hipMemset failed"));
  if (hipMalloc(&p, kVarianceStatBytes) != hipSuccess) return bail(fail(ctx, PTC_ERR_OOM, "hipMalloc(denoise variance counters) failed"));
  ctx->variance_stats = static_cast<unsigned long long*>(p);
  if (hipMemset(ctx->variance_stats, 0, kVarianceStatBytes) != hipSuccess) return bail(fail(ctx, PTC_ERR_HIP, "hipMemset failed"));
  *out = ctx;
  return PTC_OK;
}

void ptc_destroy(ptc_ctx* ctx)
{
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  for (auto& sl : ctx->slots)
    if (sl.stream) (void)hipStreamSynchronize(sl.stream);
  if (ctx->own_stream) (void)hipStreamSynchronize(ctx->own_stream);
  release_frame(*ctx);
  free_pool(ctx->scene_allocs);
  for (auto& tl : ctx->timed) {
    (void)hipEventDestroy(tl.start);
    (void)hipEventDestroy(tl.stop);
  }
  for (hipEvent_t e : ctx->free_events) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->turn_event)
    if (e) (void)hipEventDestroy(e);
  if (ctx->order_event) (void)hipEventDestroy(ctx->order_event);
  if (ctx->main_event) (void)hipEventDestroy(ctx->main_event);
  if (ctx->xstream_event) (void)hipEventDestroy(ctx->xstream_event);
  if (ctx->slot_offset_dev) (void)hipFree(ctx->slot_offset_dev);
  for (hipEvent_t e : ctx->gather_ev)
    if (e) (void)hipEventDestroy(e);
  if (ctx->misc_counters) (void)hipFree(ctx->misc_counters);
  if (ctx->loop_stats) (void)hipFree(ctx->loop_stats);
  if (ctx->albedo_stats) (void)hipFree(ctx->albedo_stats);
  if (ctx->variance_stats) (void)hipFree(ctx->variance_stats);
  if (ctx->env.texels) (void)hipFree(const_cast<float4*>(ctx->env.texels));
  if (ctx->env_table) (void)hipFree(const_cast<uint4*>(ctx->env_table));
  if (ctx->meter_dev) (void)hipFree(ctx->meter_dev);  // (exposure_dev is the same allocation)
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
}

int ptc_set_stream(ptc_ctx* ctx, void* hip_stream)
{
  if (!ctx) return PTC_ERR_INVALID;
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  ctx->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->own_stream;
  if (!ctx->staged && !ctx->slots.empty()) ctx->slots[0].stream = ctx->stream;  // one frame in flight: trace on the caller's stream
  return PTC_OK;
}

int ptc_resize(ptc_ctx* ctx, uint32_t width, uint32_t height)
{
  // ---- refusals: the frame the context has stays as it is
  if (!ctx || width < 2u || height < 2u) return fail(ctx, PTC_ERR_INVALID, "resolution must be at least 2x2");
  if ((uint64_t)width * height > 0x7fffffffull) return fail(ctx, PTC_ERR_INVALID, "too many pixels");
  if (int rc = bind_device(ctx)) return rc;
  // ---- the plan
  const ptc_frame_plan plan = frame_plan(width, height, ctx->frames_in_flight, ctx->frames_auto, ctx->batch_frames, ctx->prefold);
  // ---- the old frame goes before the new one's allocations: its memory is needed.  Iterations queued or in flight were asked
  // for at its size: trace them first.  From here to the commit the context holds no frame, and a failure leaves it so (~NewFrame)
  if (int rc = sync_frames(ctx)) return rc;
  release_frame(*ctx);
  // ---- the new frame, beside the context
  NewFrame n;
  if (int rc = build_frame(ctx, width, height, plan, n)) return rc;
  // ---- the commit: nothing above assigned a frame field of the context, nothing below can fail
  std::swap(static_cast<ptc_frame_state&>(*ctx), static_cast<ptc_frame_state&>(n));
  return ptc_restart(ctx);
}

int ptc_restart(ptc_ctx* ctx)
{
  if (!ctx) return PTC_ERR_INVALID;
  // Iterations still queued are traced first, not dropped: the reference has rendered them by the time restart()
  // runs (path_trace is synchronous there), and a present between restart and the next path_trace shows them.
  // A viewer restarts after it has presented, i.e. with an empty queue, so this costs nothing where it matters.
  if (!ctx->pending.empty() || !ctx->held.empty())
    if (int rc = flush_pending(ctx)) return rc;
  ctx->iteration = 0;
  ctx->loop_stats_clear = true;  // ptc_get_direct_loop_stats counts from here
  ctx->albedo_stage_ms = 0.0;    // ptc_get_denoise_albedo_stats' stage_ms too: launches timed before this carry the old epoch
  ctx->albedo_epoch += 1u;
  ctx->variance_stage_ms = 0.0;  // ptc_get_denoise_variance_stats' stage_ms: its launches carry the same epoch
  return PTC_OK;
}

int ptc_iteration(const ptc_ctx* ctx) { return ctx ? ctx->iteration : PTC_ERR_INVALID; }

int ptc_set_iteration(ptc_ctx* ctx, int iteration)
{
  if (!ctx || iteration < 0) return PTC_ERR_INVALID;
  if (int rc = flush_pending(ctx)) return rc;
  ctx->iteration = iteration;
  return PTC_OK;
}

int ptc_set_max_iterations(ptc_ctx* ctx, int max_iterations)
{
  if (!ctx) return PTC_ERR_INVALID;
  ctx->max_iterations = max_iterations;
  return PTC_OK;
}

int ptc_set_method(ptc_ctx* ctx, int method)
{
  if (!ctx || (method != PTC_METHOD_MEGAKERNEL && method != PTC_METHOD_STREAMING)) return fail(ctx, PTC_ERR_INVALID, "unknown method");
  if (method == ctx->method) return PTC_OK;
  if (int rc = flush_pending(ctx)) return rc;
  ctx->method = method;
  return PTC_OK;
}

int ptc_set_max_bounces(ptc_ctx* ctx, int max_bounces)
{
  if (!ctx || max_bounces < 1 || max_bounces > (int)kMaxBounces) return fail(ctx, PTC_ERR_INVALID, "max_bounces must be in [1,64]");
  if (max_bounces == ctx->max_bounces) return PTC_OK;
  if (int rc = flush_pending(ctx)) return rc;
  ctx->max_bounces = max_bounces;
  return PTC_OK;
}

int ptc_set_trace_variant(ptc_ctx* ctx, int variant)
{
  const bool known = variant == 0 || variant == 1 || variant == 3;
  if (!ctx || !known) return fail(ctx, PTC_ERR_INVALID, "unknown trace variant (0, 1 or 3)");
  if (variant == ctx->trace_variant) return PTC_OK;
  if (int rc = flush_pending(ctx)) return rc;
  ctx->trace_variant = variant;
  return PTC_OK;
}

int ptc_set_param(ptc_ctx* ctx, const char* name, int value)
{
  if (!ctx || !name) return PTC_ERR_INVALID;
  if (int rc = flush_pending(ctx)) return rc;
  // the parameters that do more than store a checked value
  if (std::strcmp(name, "slot_offset") == 0) return set_slot_offset(ctx, value);
  if (std::strcmp(name, "debug_shade_epoch") == 0) return set_shade_epoch(ctx, value);
  if (std::strcmp(name, "debug_force_slow") == 0) {  // any value; 1: every ray at fetch time, 2: every winner at verification time
    ctx->scene.force_slow = (uint32_t)value;
    ctx->force_slow = value;
    return PTC_OK;
  }
  for (const ParamRow& row : kParams) {
    if (std::strcmp(name, row.name) != 0) continue;
    if (value < row.lo || value > row.hi) return fail(ctx, PTC_ERR_INVALID, std::string(row.name) + row.complaint);
    if (row.gate == kBeforeResize && ctx->pix_capacity) return fail(ctx, PTC_ERR_INVALID, std::string("set ") + row.name + " before ptc_resize");
    if (row.gate == kBeforeUpload && ctx->has_scene) return fail(ctx, PTC_ERR_INVALID, std::string("set ") + row.name + " before ptc_upload_scene");
    row.store(ctx, value);
    // (a caller that has chosen the frames in flight gets them: ptc_resize no longer caps the count)
    if (std::strcmp(name, "frames_in_flight") == 0) ctx->frames_auto = false;
    return PTC_OK;
  }
  return fail(ctx, PTC_ERR_INVALID, std::string("unknown parameter ") + name);
}

// The thin lens.  Checked values only: a refusal leaves the context's lens as it was.
int ptc_set_lens(ptc_ctx* ctx, float lens_radius, float focus_distance)
{
  if (!ctx) return PTC_ERR_INVALID;
  if (int rc = flush_pending(ctx)) return rc;  // a batch renders with one lens
  if (!std::isfinite(lens_radius)) return fail(ctx, PTC_ERR_INVALID, "lens_radius must be finite, got " + std::to_string(lens_radius));
  if (!std::isfinite(focus_distance)) return fail(ctx, PTC_ERR_INVALID, "focus_distance must be finite, got " + std::to_string(focus_distance));
  if (lens_radius < 0.0f) return fail(ctx, PTC_ERR_INVALID, "lens_radius must not be negative, got " + std::to_string(lens_radius));
  if (lens_radius > 0.0f && !(focus_distance > 0.0f))
    return fail(ctx, PTC_ERR_INVALID, "focus_distance must be positive under a lens_radius > 0, got " + std::to_string(focus_distance));
  ctx->lens = DLens{lens_radius, focus_distance};
  return PTC_OK;
}

int ptc_get_lens(ptc_ctx* ctx, float* lens_radius, float* focus_distance)
{
  if (!ctx || !lens_radius || !focus_distance) return PTC_ERR_INVALID;
  *lens_radius = ctx->lens.radius;
  *focus_distance = ctx->lens.focus;
  return PTC_OK;
}

// The environment.  Everything that can refuse comes before the context changes: the map that was set stays in
// place after any refusal.  The new map is uploaded into an allocation of its own and the old one freed only then; frames in flight
// have read the old one by the time sync_frames returns.
int ptc_set_environment(ptc_ctx* ctx, const float* rgb, uint32_t n)
{
  if (!ctx) return PTC_ERR_INVALID;
  if (int rc = flush_pending(ctx)) return rc;  // a batch renders under one environment
  float4* dev = nullptr;
  if (rgb && n != 0u) {
    if (n < env_rules::kMinSize || n > env_rules::kMaxSize)
      return fail(ctx, PTC_ERR_INVALID, "environment size must be in [2,4096], got " + std::to_string(n));
    const size_t comps = 3u * (size_t)n * n;
    for (size_t k = 0; k < comps; ++k)
      if (!(rgb[k] >= 0.0f) || !std::isfinite(rgb[k])) {
        const size_t texel = k / 3u;
        return fail(ctx, PTC_ERR_INVALID, "environment texel (row " + std::to_string(texel / n) + ", column " + std::to_string(texel % n) + ") component " +
                                              std::to_string(k % 3u) + " must be finite and not negative, got " + std::to_string(rgb[k]));
      }
    if (int rc = bind_device(ctx)) return rc;
    const size_t texels = (size_t)(n + 2u) * (n + 2u);
    std::vector<float4> host(texels);
    env_rules::apron(rgb, n, host.data());
    if (hipMalloc(reinterpret_cast<void**>(&dev), texels * sizeof(float4)) != hipSuccess) {
      (void)hipGetLastError();
      return fail(ctx, PTC_ERR_OOM, "hipMalloc(environment, " + std::to_string(texels * sizeof(float4)) + " bytes) failed");
    }
    const hipError_t e = hipMemcpy(dev, host.data(), texels * sizeof(float4), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(dev);
      return fail(ctx, PTC_ERR_HIP, std::string("environment upload: ") + hipGetErrorString(e));
    }
  } else if (int rc = bind_device(ctx)) {
    return rc;
  }
  if (ctx->env.texels) {  // the frames that read the old map have to be done with it
    if (int rc = sync_frames(ctx)) {
      if (dev) (void)hipFree(dev);
      return rc;
    }
    (void)hipFree(const_cast<float4*>(ctx->env.texels));
    if (ctx->env_table) (void)hipFree(const_cast<uint4*>(ctx->env_table));  // the old map's alias table goes with it
  }
  ctx->env = DEnv{dev, dev ? n : 0u, 0u};
  ctx->env_table = nullptr;
  ctx->env_table_known = false;
  return PTC_OK;
}

}  // extern "C"

// The environment's alias table, at the first call that needs it: the aproned map comes back from the device (the
// host keeps no copy of it), env_light::build_table makes the entries, and they are uploaded into an allocation of their own.
// Nothing reads the table before this returns, and nothing but ptc_set_environment and ptc_destroy frees it.
int ptcd::env_light_table(ptc_ctx* ctx)
{
  if (ctx->env_table_known || !ctx->env.texels) return PTC_OK;
  const uint32_t n = ctx->env.n;
  std::vector<float4> host((size_t)(n + 2u) * (n + 2u));
  HIP_TRY(ctx, hipMemcpy(host.data(), ctx->env.texels, host.size() * sizeof(float4), hipMemcpyDeviceToHost));
  std::vector<env_light::Entry> entries;
  if (env_light::build_table(host.data(), n, entries, nullptr) > 0.0) {
    const size_t bytes = entries.size() * sizeof(env_light::Entry);
    void* dev = nullptr;
    if (hipMalloc(&dev, bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail(ctx, PTC_ERR_OOM, "hipMalloc(environment light table, " + std::to_string(bytes) + " bytes) failed");
    }
    const hipError_t e = hipMemcpy(dev, entries.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(dev);
      return fail(ctx, PTC_ERR_HIP, std::string("environment light table upload: ") + hipGetErrorString(e));
    }
    ctx->env_table = static_cast<const uint4*>(dev);
  }
  ctx->env_table_known = true;
  return PTC_OK;
}

extern "C" {

// An equirectangular image to the octahedral map ptc_set_environment takes (host only; float64 inside, not parity-critical).  Per
// octahedral texel centre: the direction, the image sampled bilinearly at u = atan2(d.x, -d.z) / 2 pi + 0.5 (wrapping) and v =
// acos(d.y) / pi (clamping) -- the image's centre is the camera's default view direction -z, row 0 is up --, times scale, to binary32.
// A point sample per texel: a map much smaller than the image skips pixels (a small sun may fall between texels).
int ptc_environment_from_equirect(const float* rgb, uint32_t width, uint32_t height, uint32_t n, float scale, float* out)
{
  if (!rgb || !out || width == 0u || height == 0u || n < env_rules::kMinSize || n > env_rules::kMaxSize) return PTC_ERR_INVALID;
  if (!std::isfinite(scale) || scale < 0.0f) return PTC_ERR_INVALID;
  const double pi = 3.14159265358979323846;
  for (uint32_t j = 0; j < n; ++j)
    for (uint32_t i = 0; i < n; ++i) {
      const double qx = 2.0 * (((double)i + 0.5) / (double)n) - 1.0, qz = 2.0 * (((double)j + 0.5) / (double)n) - 1.0;
      double x = qx, z = qz;
      const double y = 1.0 - std::fabs(qx) - std::fabs(qz);
      if (y < 0.0) {  // the lower hemisphere, unfolded (the inverse of env_rules::locate's fold)
        x = (1.0 - std::fabs(qz)) * (qx < 0.0 ? -1.0 : 1.0);
        z = (1.0 - std::fabs(qx)) * (qz < 0.0 ? -1.0 : 1.0);
      }
      const double len = std::sqrt(x * x + y * y + z * z);
      const double u = std::atan2(x / len, -z / len) / (2.0 * pi) + 0.5;
      const double v = std::acos(std::min(1.0, std::max(-1.0, y / len))) / pi;
      const double fx = u * (double)width - 0.5, fy = v * (double)height - 0.5;
      const double x0f = std::floor(fx), y0f = std::floor(fy);
      const double tx = fx - x0f, ty = fy - y0f;
      const int64_t W = (int64_t)width, Hh = (int64_t)height;
      const int64_t x0 = (((int64_t)x0f % W) + W) % W, x1 = (x0 + 1) % W;
      const int64_t y0 = std::min<int64_t>(std::max<int64_t>((int64_t)y0f, 0), Hh - 1), y1 = std::min<int64_t>(std::max<int64_t>((int64_t)y0f + 1, 0), Hh - 1);
      for (int c = 0; c < 3; ++c) {
        const double c00 = rgb[3 * (y0 * W + x0) + c], c10 = rgb[3 * (y0 * W + x1) + c];
        const double c01 = rgb[3 * (y1 * W + x0) + c], c11 = rgb[3 * (y1 * W + x1) + c];
        const double top = c00 * (1.0 - tx) + c10 * tx, bot = c01 * (1.0 - tx) + c11 * tx;
        out[3 * ((size_t)j * n + i) + c] = (float)((top * (1.0 - ty) + bot * ty) * (double)scale);
      }
    }
  return PTC_OK;
}

int ptc_get_environment(ptc_ctx* ctx, uint32_t* n)
{
  if (!ctx || !n) return PTC_ERR_INVALID;
  *n = ctx->env.n;
  return PTC_OK;
}

int ptc_set_denoiser_params(ptc_ctx* ctx, const ptc_denoiser_params* p)
{
  if (!ctx || !p) return PTC_ERR_INVALID;
  ctx->den = *p;
  return PTC_OK;
}

// what ptc_denoise and ptc_denoise_albedo refuse, in the one order they share
static int denoise_ready(ptc_ctx* ctx)
{
  if (int rc = frame_ready(ctx)) return rc;
  if (!ctx->have_cam) return fail(ctx, PTC_ERR_INVALID, "denoise needs a traced frame (it reuses the last camera)");
  if (ctx->pix_count != ctx->width * ctx->height) return fail(ctx, PTC_ERR_INVALID, "denoise needs the full frame in one context");
  return PTC_OK;
}

// "denoise_albedo" (DESIGN section 5r): the two planes of this frame size, allocated by the first call that gets here and released
// with the frame (release_frame: they are of frame_allocs)
static int albedo_planes(ptc_ctx* ctx)
{
  static_assert(kDenoiseAlbedoPlanes == 2, "the albedo and the irradiance plane");
  const size_t elems = (size_t)denoise_albedo_floats4(ctx->width, ctx->height);
  if (!ctx->den_albedo)
    if (int rc = dev_alloc(ctx, ctx->frame_allocs, &ctx->den_albedo, elems)) return rc;
  if (!ctx->den_irradiance)
    if (int rc = dev_alloc(ctx, ctx->frame_allocs, &ctx->den_irradiance, elems)) return rc;
  return PTC_OK;
}

// Stages 1 and 2 on ctx->stream: the counter block zeroed, then k_denoise_albedo over the accumulated colour under the textures the
// megakernel would use now (`textured` of mega_frame, ptcore_trace.cpp: "textures" with textures and coordinates set; else none).
// rays: null, or 2 float4 a pixel on the device.  Timed as one launch of the stage.
static int albedo_stage(ptc_ctx* ctx, float4* rays)
{
  const bool textured = ctx->textures && ctx->textures_set && ctx->texcoords_set;
  const DTex tx = textured ? DTex{ctx->tex_texels, ctx->tex_records, ctx->tex_material, ctx->tex_table, ctx->texcoords, ctx->mesh_first_index} : DTex{};
  HIP_TRY(ctx, hipMemsetAsync(ctx->albedo_stats, 0, kLoopStatBytes, ctx->stream));
  ptc_ctx::TimedLaunch tl;
  if (int rc = timed_begin(ctx, ctx->stream, -2, &tl)) return rc;
  tl.tag = ctx->albedo_epoch;
  launch_denoise_albedo(ctx->stream, ctx->scene, tx, ctx->cam, ctx->fb.color4, ctx->den_albedo, ctx->den_irradiance, rays, ctx->albedo_stats,
                        &ctx->misc_counters->flags);
  return timed_end(ctx, ctx->stream, tl);
}

// "denoise_variance" (DESIGN section 5s): the two variance planes of this frame size, allocated by the first call that gets here and
// released with the frame (release_frame: they are of frame_allocs)
static int variance_planes(ptc_ctx* ctx)
{
  static_assert(kDenoiseVariancePlanes == 2, "the variance planes that ping-pong beside den_a and den_b");
  const size_t elems = (size_t)denoise_variance_floats(ctx->width, ctx->height);
  if (!ctx->den_var_a)
    if (int rc = dev_alloc(ctx, ctx->frame_allocs, &ctx->den_var_a, elems)) return rc;
  if (!ctx->den_var_b)
    if (int rc = dev_alloc(ctx, ctx->frame_allocs, &ctx->den_var_b, elems)) return rc;
  return PTC_OK;
}

// The estimate stage on ctx->stream: the counters zeroed, k_variance_estimate of `plane` (under the normals and den_pos, which the
// caller has made) into den_var_a, then k_variance_prefilter of that, which counts the pixels on the floor and, for
// ptc_denoise_variance (keep_prefiltered), writes the prefiltered plane into den_var_b; under ptc_denoise it writes nothing -- the
// passes prefilter for themselves.  Timed as one launch of the stage.
static int variance_stage(ptc_ctx* ctx, const float4* plane, bool keep_prefiltered)
{
  HIP_TRY(ctx, hipMemsetAsync(ctx->variance_stats, 0, kVarianceStatBytes, ctx->stream));
  ptc_ctx::TimedLaunch tl;
  if (int rc = timed_begin(ctx, ctx->stream, -3, &tl)) return rc;
  tl.tag = ctx->albedo_epoch;
  launch_variance_estimate(ctx->stream, ctx->width, ctx->height, plane, ctx->fb.nd4, ctx->den_pos, ctx->den_var_a, ctx->den.normal_weight,
                           ctx->den.position_weight);
  launch_variance_prefilter(ctx->stream, ctx->width, ctx->height, ctx->den_var_a, keep_prefiltered ? ctx->den_var_b : nullptr,
                            ctx->variance_stats);
  return timed_end(ctx, ctx->stream, tl);
}

int ptc_denoise(ptc_ctx* ctx)
{
  if (int rc = denoise_ready(ctx)) return rc;
  if (int rc = flush_pending(ctx)) return rc;
  // "denoise_albedo": the passes filter the irradiance plane and their result is multiplied back (no pass, no stage)
  const bool albedo = ctx->denoise_albedo && ctx->den.filter_size >= 1;
  if (albedo)
    if (int rc = albedo_planes(ctx)) return rc;
  // "denoise_variance": an estimate stage ahead of the passes, and the guided passes in the plain ones' place (no pass, no stage)
  const bool guided = ctx->denoise_variance && ctx->den.filter_size >= 1;
  if (guided)
    if (int rc = variance_planes(ctx)) return rc;
  // every sample must be folded in before the framebuffers are read (stream order, no host sync)
  if (ctx->order_valid) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->order_event, 0));
  else if (!ctx->slots.empty() && ctx->slots[(size_t)ctx->last_slot].stream != ctx->stream)
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->slots[(size_t)ctx->last_slot].done, 0));
  const DDenoise prm{ctx->den.color_weight, ctx->den.normal_weight, ctx->den.position_weight, ctx->denoise_variant};
  // edge_avoiding_a_trous_denoiser.cu:102-108: (color, back, front) <- (back, front, back) after each pass
  const float4* color = ctx->fb.color4;
  float4* back = ctx->den_a;
  float4* front = ctx->den_b;
  if (ctx->den.filter_size >= 1) launch_denoise_positions(ctx->stream, ctx->cam, ctx->pix_count, ctx->fb.nd4, ctx->den_pos);
  if (albedo) {
    if (int rc = albedo_stage(ctx, nullptr)) return rc;
    color = ctx->den_irradiance;
  }
  // (guided only) the variance travels beside the colour: (var, var_back) swap as (color, back) do
  DDenoiseVar vprm{};
  const float* var = nullptr;
  float* var_back = nullptr;
  if (guided) {
    vprm = DDenoiseVar{ctx->den.normal_weight, ctx->den.position_weight, ctx->variance_sigma, ctx->denoise_variant};
    var = ctx->den_var_a;
    var_back = ctx->den_var_b;
    if (int rc = variance_stage(ctx, color, false)) return rc;
  }
  for (int step = 1; step <= ctx->den.filter_size; step *= 2) {
    ptc_ctx::TimedLaunch tl;
    if (int rc = timed_begin(ctx, ctx->stream, -1, &tl)) return rc;
    if (guided) {
      launch_denoise_var_pass(ctx->stream, ctx->cam, ctx->pix_count, color, var, ctx->fb.nd4, ctx->den_pos, back, var_back, step, vprm);
      float* const written = var_back;
      var_back = const_cast<float*>(var);
      var = written;
    } else {
      launch_denoise_pass(ctx->stream, ctx->cam, ctx->pix_count, color, ctx->fb.nd4, ctx->den_pos, back, step, prm);
    }
    if (int rc = timed_end(ctx, ctx->stream, tl)) return rc;
    const float4* new_color = back;
    float4* new_back = front;
    float4* new_front = back;
    color = new_color;
    back = new_back;
    front = new_front;
  }
  if (albedo) {  // (filter_size >= 1: front is the last pass's output)
    ptc_ctx::TimedLaunch tl;
    if (int rc = timed_begin(ctx, ctx->stream, -2, &tl)) return rc;
    tl.tag = ctx->albedo_epoch;
    launch_remodulate(ctx->stream, ctx->pix_count, ctx->den_albedo, front);
    if (int rc = timed_end(ctx, ctx->stream, tl)) return rc;
  }
  ctx->result = front;
  if (int rc = check_last(ctx, "denoise")) return rc;
  HIP_TRY(ctx, hipEventRecord(ctx->main_event, ctx->stream));
  ctx->main_valid = true;
  return PTC_OK;
}

int ptc_present_rgba8(ptc_ctx* ctx, void* dst, int dst_is_device, int display_type)
{
  if (int rc = view_ready(ctx, dst)) return rc;
  if (int rc = flush_pending(ctx)) return rc;
  DisplayView show;
  BufferView view;
  if (int rc = display_view(ctx, display_type, false, &show)) return rc;
  if (int rc = buffer_view(ctx, show.which, &view)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  uint32_t* out = dst_is_device ? static_cast<uint32_t*>(dst) : ctx->rgba_buf;
  // radiance under a display of the context's; the reference display and the other views: k_preview, as ever
  const bool displayed = show.mode == 0 && !reference_display(ctx->display);
  if (displayed) {
    if (int rc = show_display(ctx, view.src, nullptr, ctx->pix_count, out, nullptr, &ctx->shown)) return rc;
  } else {
    launch_preview(ctx->stream, view.src, ctx->pix_count, show.mode, out);
    if (int rc = check_last(ctx, "preview")) return rc;
  }
  if (!dst_is_device)
    HIP_TRY(ctx, hipMemcpyAsync(dst, ctx->rgba_buf, (size_t)ctx->pix_count * 4u, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // path_tracer.cu:519
  if (displayed) ctx->shown_known = true;
  return PTC_OK;
}

int ptc_download(ptc_ctx* ctx, int which, void* dst, int dst_is_device)
{
  if (int rc = view_ready(ctx, dst)) return rc;
  if (int rc = flush_pending(ctx)) return rc;
  BufferView view;
  if (int rc = buffer_view(ctx, which, &view)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  float* out = dst_is_device ? static_cast<float*>(dst) : ctx->pack_buf;
  launch_pack(ctx->stream, view.src, ctx->pix_count, view.sel, out);
  if (int rc = check_last(ctx, "pack")) return rc;
  const size_t floats = (size_t)ctx->pix_count * view.floats_per_pixel;
  if (!dst_is_device) HIP_TRY(ctx, hipMemcpyAsync(dst, ctx->pack_buf, floats * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return PTC_OK;
}

int ptc_synchronize(ptc_ctx* ctx)
{
  if (!ctx) return PTC_ERR_INVALID;
  if (int rc = bind_device(ctx)) return rc;
  return sync_frames(ctx);
}

int ptc_get_stats(ptc_ctx* ctx, ptc_stats* out)
{
  if (!ctx || !out) return PTC_ERR_INVALID;
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  std::memset(out, 0, sizeof *out);
  uint32_t flags = 0;
  if (int rc = each_counter_head(ctx, [&](size_t f, int k, const DeviceCounters& host) {
        out->rays_total += host.rays_total;
        flags |= host.flags;
        if ((int)f == ctx->last_slot && k + 1 == (int)ctx->slots[f].bi.count)
          for (int i = 0; i < PTC_MAX_BOUNCES_CAP; ++i) out->last_live[i] = i < ctx->max_bounces ? host.live[i] : 0u;
      }))
    return rc;
  std::vector<char> buf(sizeof(DeviceCounters));
  HIP_TRY(ctx, hipMemcpy(buf.data(), ctx->misc_counters, kCountersHead, hipMemcpyDeviceToHost));
  flags |= reinterpret_cast<const DeviceCounters*>(buf.data())->flags;
  out->frames = ctx->frames;
  out->bvh_node_count = ctx->bvh_nodes;
  out->bvh_max_depth = ctx->bvh_depth;
  out->triangle_count = ctx->triangles;
  out->stack_capacity = kStackDepth;
  if (flags & kFlagStackOverflow) return fail(ctx, PTC_ERR_STACK, "traversal stack overflow during rendering");
  if (flags & kFlagPersistStall)
    return fail(ctx, PTC_ERR_HIP, "the persistent launch (k_persist) gave up waiting for work: a wavefront of its batch never finished (\"persist\" 0 turns it off)");
  if (flags & kFlagDispatchOrder)
    return fail(ctx, PTC_ERR_HIP, "k_shade_fused gave up waiting for a predecessor tile's survivor count: the image is invalid "
                                  "(set the parameter \"fused_shade\" to 0 to use the three-kernel path)");
  return PTC_OK;
}

int ptc_get_direct_loop_stats(ptc_ctx* ctx, ptc_direct_loop_stats* out)
{
  if (!ctx || !out) return PTC_ERR_INVALID;
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  *out = ptc_direct_loop_stats{};
  if (ctx->loop_stats_clear) return PTC_OK;  // nothing direct-lit has been launched since ptc_restart
  std::vector<unsigned long long> host((size_t)kLightStatLines * kLoopStatWords);
  HIP_TRY(ctx, hipMemcpy(host.data(), ctx->loop_stats, kLoopStatBytes, hipMemcpyDeviceToHost));
  for (uint32_t l = 0; l < kLightStatLines; ++l) {
    out->diffuse_hits += host[(size_t)kLoopStatWords * l];
    out->shadow_rays += host[(size_t)kLoopStatWords * l + 1u];
    out->unoccluded += host[(size_t)kLoopStatWords * l + 2u];
  }
  return PTC_OK;
}

int ptc_get_environment_light_loop_stats(ptc_ctx* ctx, ptc_environment_light_loop_stats* out)
{
  if (!ctx || !out) return PTC_ERR_INVALID;
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  *out = ptc_environment_light_loop_stats{};
  if (ctx->loop_stats_clear) return PTC_OK;  // nothing that counts has been launched since ptc_restart
  std::vector<unsigned long long> host((size_t)kLightStatLines * kLoopStatWords);
  HIP_TRY(ctx, hipMemcpy(host.data(), ctx->loop_stats, kLoopStatBytes, hipMemcpyDeviceToHost));
  for (uint32_t l = 0; l < kLightStatLines; ++l) {
    out->diffuse_hits += host[(size_t)kLoopStatWords * l + 3u];
    out->shadow_rays += host[(size_t)kLoopStatWords * l + 4u];
    out->unoccluded += host[(size_t)kLoopStatWords * l + 5u];
  }
  return PTC_OK;
}

int ptc_get_mis_loop_stats(ptc_ctx* ctx, ptc_mis_loop_stats* out)
{
  if (!ctx || !out) return PTC_ERR_INVALID;
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  *out = ptc_mis_loop_stats{};
  if (ctx->loop_stats_clear) return PTC_OK;  // nothing that counts has been launched since ptc_restart
  std::vector<unsigned long long> host((size_t)kLightStatLines * kLoopStatWords);
  HIP_TRY(ctx, hipMemcpy(host.data(), ctx->loop_stats, kLoopStatBytes, hipMemcpyDeviceToHost));
  for (uint32_t l = 0; l < kLightStatLines; ++l) {
    out->weighted_emitter_hits += host[(size_t)kLoopStatWords * l + 6u];
    out->weighted_misses += host[(size_t)kLoopStatWords * l + 7u];
  }
  return PTC_OK;
}

int ptc_get_smooth_loop_stats(ptc_ctx* ctx, ptc_smooth_loop_stats* out)
{
  if (!ctx || !out) return PTC_ERR_INVALID;
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  *out = ptc_smooth_loop_stats{};
  if (ctx->loop_stats_clear) return PTC_OK;  // nothing that counts has been launched since ptc_restart
  std::vector<unsigned long long> host((size_t)kLightStatLines * kLoopStatWords);
  HIP_TRY(ctx, hipMemcpy(host.data(), ctx->loop_stats, kLoopStatBytes, hipMemcpyDeviceToHost));
  for (uint32_t l = 0; l < kLightStatLines; ++l) {
    out->shading_normals += host[(size_t)kLoopStatWords * l + 8u];
    out->fallbacks += host[(size_t)kLoopStatWords * l + 9u];
    out->absorbed += host[(size_t)kLoopStatWords * l + 10u];
    out->culled_light_samples += host[(size_t)kLoopStatWords * l + 11u];
  }
  return PTC_OK;
}

int ptc_get_texture_loop_stats(ptc_ctx* ctx, ptc_texture_loop_stats* out)
{
  if (!ctx || !out) return PTC_ERR_INVALID;
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  *out = ptc_texture_loop_stats{};
  if (ctx->loop_stats_clear) return PTC_OK;  // nothing that counts has been launched since ptc_restart
  std::vector<unsigned long long> host((size_t)kLightStatLines * kLoopStatWords);
  HIP_TRY(ctx, hipMemcpy(host.data(), ctx->loop_stats, kLoopStatBytes, hipMemcpyDeviceToHost));
  for (uint32_t l = 0; l < kLightStatLines; ++l) {
    out->lookups += host[(size_t)kLoopStatWords * l + 12u];
    out->fallbacks += host[(size_t)kLoopStatWords * l + 13u];
  }
  return PTC_OK;
}

int ptc_get_normal_map_loop_stats(ptc_ctx* ctx, ptc_normal_map_loop_stats* out)
{
  if (!ctx || !out) return PTC_ERR_INVALID;
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  *out = ptc_normal_map_loop_stats{};
  if (ctx->loop_stats_clear) return PTC_OK;  // nothing that counts has been launched since ptc_restart
  std::vector<unsigned long long> host((size_t)kLightStatLines * kLoopStatWords);
  HIP_TRY(ctx, hipMemcpy(host.data(), ctx->loop_stats, kLoopStatBytes, hipMemcpyDeviceToHost));
  for (uint32_t l = 0; l < kLightStatLines; ++l) {
    out->bent += host[(size_t)kLoopStatWords * l + 14u];
    out->kept += host[(size_t)kLoopStatWords * l + 15u];
  }
  return PTC_OK;
}

static int drain_timed(ptc_ctx* ctx)
{
  for (auto& tl : ctx->timed) {
    float ms = 0.0f;
    HIP_TRY(ctx, hipEventSynchronize(tl.stop));
    HIP_TRY(ctx, hipEventElapsedTime(&ms, tl.start, tl.stop));
    if (tl.bounce == -2) {
      if (tl.tag == ctx->albedo_epoch) ctx->albedo_stage_ms += ms;
    } else if (tl.bounce == -3) {
      if (tl.tag == ctx->albedo_epoch) ctx->variance_stage_ms += ms;
    } else if (tl.bounce < 0) {
      ctx->denoise_ms += ms;
      ctx->denoise_passes += 1u;
    } else {
      ctx->trace_ms[tl.bounce] += ms;
      ctx->trace_launches[tl.bounce] += 1u;
    }
    ctx->free_events.push_back(tl.start);
    ctx->free_events.push_back(tl.stop);
  }
  ctx->timed.clear();
  return PTC_OK;
}

int ptc_set_profiling(ptc_ctx* ctx, int time_trace_kernel, int count_tests)
{
  if (!ctx) return PTC_ERR_INVALID;
  ctx->time_trace = time_trace_kernel != 0;
  ctx->count_tests = count_tests != 0;
  return PTC_OK;
}

int ptc_reset_profile(ptc_ctx* ctx)
{
  if (!ctx) return PTC_ERR_INVALID;
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  if (int rc = drain_timed(ctx)) return rc;
  std::memset(ctx->trace_ms, 0, sizeof ctx->trace_ms);
  std::memset(ctx->trace_launches, 0, sizeof ctx->trace_launches);
  ctx->denoise_ms = 0.0;
  ctx->denoise_passes = 0;
  ctx->persist_launches = 0;
  ctx->intersect_redone = 0;
  ctx->occlusion = ptc_occlusion_stats{};
  ctx->direct = ptc_direct_stats{};
  ctx->env_direct = ptc_environment_light_stats{};
  const size_t off = offsetof(DeviceCounters, paths);  // the profile counters: from `paths` to the end of the head
  return each_counter_block(ctx, [&](size_t, int, DeviceCounters* dev) -> int {
    HIP_TRY(ctx, hipMemset(reinterpret_cast<char*>(dev) + off, 0, kCountersHead - off));
    return PTC_OK;
  });
}

int ptc_get_profile(ptc_ctx* ctx, ptc_profile* out)
{
  if (!ctx || !out) return PTC_ERR_INVALID;
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  if (int rc = drain_timed(ctx)) return rc;
  std::memset(out, 0, sizeof *out);
  if (int rc = each_counter_head(ctx, [&](size_t, int, const DeviceCounters& host) {
        for (int b = 0; b < PTC_MAX_BOUNCES_CAP; ++b) {
          out->paths[b] += host.paths[b];
          out->box_tests[b] += host.box_tests[b];
          out->tri_tests[b] += host.tri_tests[b];
          out->max_box_tests[b] = std::max(out->max_box_tests[b], host.max_box_tests[b]);
          out->listed_rays[b] += host.listed_rays[b];
          out->slow_rays[b] += host.slow_rays[b];
          out->node_visits[b] += host.node_visits[b];
        }
      }))
    return rc;
  for (int b = 0; b < PTC_MAX_BOUNCES_CAP; ++b) {
    out->trace_ms[b] = ctx->trace_ms[b];
    out->trace_launches[b] = ctx->trace_launches[b];
  }
  out->slow_rays[0] += ctx->intersect_redone;
  out->denoise_ms = ctx->denoise_ms;
  out->denoise_passes = ctx->denoise_passes;
  out->persist_launches = ctx->persist_launches;
  return PTC_OK;
}

// Stages 1 and 2 of "denoise_albedo" alone, whatever the parameter says: the planes and the rays the kernel built,
// packed to the caller's host arrays.  The frames in flight are folded in first (host-side, as ptc_download does).
int ptc_denoise_albedo(ptc_ctx* ctx, float* albedo_out, float* irradiance_out, float* rays_out)
{
  if (int rc = denoise_ready(ctx)) return rc;
  if (int rc = flush_pending(ctx)) return rc;
  if (int rc = albedo_planes(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  const size_t P = ctx->pix_count;
  std::vector<void*> pool;
  float4* d_rays = nullptr;
  auto run = [&]() -> int {
    if (rays_out)
      if (int rc = dev_alloc(ctx, pool, &d_rays, 2u * P)) return rc;
    if (int rc = albedo_stage(ctx, d_rays)) return rc;
    if (int rc = check_last(ctx, "denoise_albedo")) return rc;
    for (const auto& plane : {std::make_pair((const float4*)ctx->den_albedo, albedo_out), std::make_pair((const float4*)ctx->den_irradiance, irradiance_out)}) {
      if (!plane.second) continue;
      launch_pack(ctx->stream, plane.first, ctx->pix_count, 0, ctx->pack_buf);  // (stream order: the copy below is done before the next pack)
      if (int rc = check_last(ctx, "pack")) return rc;
      HIP_TRY(ctx, hipMemcpyAsync(plane.second, ctx->pack_buf, 3u * P * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (rays_out) HIP_TRY(ctx, hipMemcpyAsync(rays_out, d_rays, 2u * P * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    return PTC_OK;
  };
  const int rc = run();
  const hipError_t e = hipStreamSynchronize(ctx->stream);  // nothing may still use the pool; the caller's arrays are complete
  free_pool(pool);
  if (rc) return rc;
  if (e != hipSuccess) return fail(ctx, PTC_ERR_HIP, std::string("denoise_albedo: ") + hipGetErrorString(e));
  return PTC_OK;
}

int ptc_get_denoise_albedo_stats(ptc_ctx* ctx, ptc_denoise_albedo_stats* out)
{
  if (!ctx || !out) return PTC_ERR_INVALID;
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  if (int rc = drain_timed(ctx)) return rc;
  *out = ptc_denoise_albedo_stats{};
  std::vector<unsigned long long> host((size_t)kLightStatLines * kLoopStatWords);
  HIP_TRY(ctx, hipMemcpy(host.data(), ctx->albedo_stats, kLoopStatBytes, hipMemcpyDeviceToHost));
  for (uint32_t l = 0; l < kLightStatLines; ++l) {
    out->pixels += host[(size_t)kLoopStatWords * l];
    out->surface_hits += host[(size_t)kLoopStatWords * l + 1u];
    out->texel_lookups += host[(size_t)kLoopStatWords * l + 2u];
    out->floored += host[(size_t)kLoopStatWords * l + 3u];
  }
  out->stage_ms = ctx->albedo_stage_ms;
  return PTC_OK;
}

int ptc_set_denoise_variance(ptc_ctx* ctx, float sigma)
{
  if (!ctx) return PTC_ERR_INVALID;
  if (!std::isfinite(sigma) || !(sigma > 0.0f)) return fail(ctx, PTC_ERR_INVALID, "denoise_variance: sigma must be finite and > 0");
  ctx->variance_sigma = sigma;
  return PTC_OK;
}

int ptc_get_denoise_variance(ptc_ctx* ctx, float* sigma)
{
  if (!ctx || !sigma) return PTC_ERR_INVALID;
  *sigma = ctx->variance_sigma;
  return PTC_OK;
}

// The estimate stage of "denoise_variance" alone, whatever the parameter says, on the plane ptc_denoise would
// filter now: the irradiance under "denoise_albedo" 1 (the albedo stage runs first), else the accumulated colour.  The frames in
// flight are folded in first (host-side, as ptc_download does).
int ptc_denoise_variance(ptc_ctx* ctx, float* variance_out, float* prefiltered_out)
{
  if (int rc = denoise_ready(ctx)) return rc;
  if (int rc = flush_pending(ctx)) return rc;
  if (ctx->denoise_albedo)
    if (int rc = albedo_planes(ctx)) return rc;
  if (int rc = variance_planes(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  const size_t P = ctx->pix_count;
  auto run = [&]() -> int {
    launch_denoise_positions(ctx->stream, ctx->cam, ctx->pix_count, ctx->fb.nd4, ctx->den_pos);
    const float4* plane = ctx->fb.color4;
    if (ctx->denoise_albedo) {
      if (int rc = albedo_stage(ctx, nullptr)) return rc;
      plane = ctx->den_irradiance;
    }
    if (int rc = variance_stage(ctx, plane, true)) return rc;
    if (int rc = check_last(ctx, "denoise_variance")) return rc;
    if (variance_out) HIP_TRY(ctx, hipMemcpyAsync(variance_out, ctx->den_var_a, P * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (prefiltered_out) HIP_TRY(ctx, hipMemcpyAsync(prefiltered_out, ctx->den_var_b, P * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return PTC_OK;
  };
  const int rc = run();
  const hipError_t e = hipStreamSynchronize(ctx->stream);  // the caller's arrays are complete
  if (rc) return rc;
  if (e != hipSuccess) return fail(ctx, PTC_ERR_HIP, std::string("denoise_variance: ") + hipGetErrorString(e));
  return PTC_OK;
}

int ptc_get_denoise_variance_stats(ptc_ctx* ctx, ptc_denoise_variance_stats* out)
{
  if (!ctx || !out) return PTC_ERR_INVALID;
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = sync_frames(ctx)) return rc;
  if (int rc = drain_timed(ctx)) return rc;
  *out = ptc_denoise_variance_stats{};
  std::vector<unsigned long long> host((size_t)kLightStatLines * kLoopStatWords);
  HIP_TRY(ctx, hipMemcpy(host.data(), ctx->variance_stats, kVarianceStatBytes, hipMemcpyDeviceToHost));
  for (uint32_t l = 0; l < kLightStatLines; ++l) {
    out->pixels += host[(size_t)kLoopStatWords * l];
    out->floored += host[(size_t)kLoopStatWords * l + 1u];
  }
  out->stage_ms = ctx->variance_stage_ms;
  return PTC_OK;
}

}  // extern "C"

