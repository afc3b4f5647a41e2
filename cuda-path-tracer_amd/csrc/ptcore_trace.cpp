// ptcore_trace.cpp -- the launch plan of a batch of frames (batch_begin / batch_bounce / batch_end), ptc_trace and its stepwise
// form, the live counts.  Part of libptcore.so (ptcore_ctx.hpp).  The ray queries outside the render loop: ptcore_query.cpp.
#include "ptcore_ctx.hpp"
#include "pt_mega_rules.hpp"

using namespace pt;
using namespace ptcd;

namespace {

// "direct_light" 1 outside the megakernel method: the refusal of ptc_trace and ptc_trace_begin
constexpr const char* kDirectNeedsMegakernel =
    "direct_light is rendered by the megakernel method only (ptc_set_method(PTC_METHOD_MEGAKERNEL)); the streaming loop has no direct lighting";
// ... and "environment_light" 1
const char* const kEnvLightNeedsMegakernel =
    "environment_light is rendered by the megakernel method only (ptc_set_method(PTC_METHOD_MEGAKERNEL)); the streaming loop has no direct lighting";
// ... and "mis" 1
const char* const kMisNeedsMegakernel =
    "mis is rendered by the megakernel method only (ptc_set_method(PTC_METHOD_MEGAKERNEL)); the streaming loop has no direct lighting";
// ... and "smooth_normals" 1
const char* const kSmoothNeedsMegakernel =
    "smooth_normals is rendered by the megakernel method only (ptc_set_method(PTC_METHOD_MEGAKERNEL)); the streaming loop shades with face normals";
// ... and "textures" 1
const char* const kTexturesNeedMegakernel =
    "textures are rendered by the megakernel method only (ptc_set_method(PTC_METHOD_MEGAKERNEL)); the streaming loop's hit records carry no primitive";
// ... and "normal_maps" 1
const char* const kNormalMapsNeedMegakernel =
    "normal_maps are rendered by the megakernel method only (ptc_set_method(PTC_METHOD_MEGAKERNEL)); the streaming loop's hit records carry no primitive";

// the epoch of the next look-back launch on a slot's tile descriptors (k_shade_fused, the listing k_raygen / k_spheres).  After
// kMaxEpoch the epochs start at 1 again, and a descriptor that no launch of the finished lap has overwritten (a tile above a band
// that ptc_set_rows shrank) would pass for one of the new lap: the descriptors are cleared on the slot's stream, behind the last
// launch of the old lap and in front of the launch that takes epoch 1.  (A failure of the clear is the caller's next check_last.)
uint32_t next_epoch(ptc_ctx::FrameSlot& sl)
{
  if (sl.shade_epoch >= kMaxEpoch) {
    (void)hipMemsetAsync(sl.tile_desc, 0, sizeof(unsigned long long) * (size_t)sl.capacity * sl.tile_stride, sl.stream);
    sl.shade_epoch = 0u;
  }
  return ++sl.shade_epoch;
}

// Persistent wavefronts of a traversal launch.  A launch ends with its longest ray (about 100 us however few rays it
// carries), so a small launch wants about one ray per lane -- rays / 64 wavefronts, at least 1024, at most 3072 -- and
// only a launch with eight or more rays per lane fills every wavefront slot of the chip (traverse_waves: what is
// resident at five per SIMD).  Measured on single 1080p frames (2 M rays at the first bounce, 65 k at the eighth): one size
// for all bounces 2.60 ms per frame, sized per bounce 2.1 ms.  The ray count of a bounce lives on the device; the
// host sizes with the counts of a recent frame (FrameSlot::live_host), a bounce it knows nothing about with its cap.
uint32_t traverse_waves_for(ptc_ctx* ctx, uint32_t frames, int bounce, bool listed, bool run = false)
{
  for (auto& sl : ctx->slots)
    if (sl.live_pending && sl.done && hipEventQuery(sl.done) == hipSuccess) {
      std::memcpy(ctx->est_live, sl.live_host, sizeof ctx->est_live);
      ctx->est_valid = true;
      sl.live_pending = false;
    }
  (void)hipGetLastError();  // hipEventQuery's "not ready" is no error
  uint64_t per_frame = ctx->pix_count;
  if (ctx->est_valid && ctx->est_live[0] == ctx->pix_count) per_frame = std::min<uint64_t>(ctx->pix_count, ctx->est_live[bounce]);
  // a launch that walks a work list carries the listed rays only (a single frame's primary rays: 0.85 of 2.07 M on the
  // benchmark scene -- 2.6 rays per lane of a full launch, and the smaller launch ends sooner)
  if (listed && ctx->est_valid && ctx->est_live[0] == ctx->pix_count && ctx->est_live[kMaxBounces + 1 + bounce] != 0u)
    per_frame = std::min<uint64_t>(per_frame, (uint64_t)ctx->est_live[kMaxBounces + 1 + bounce] * 9u / 8u + 64u);
  const uint64_t rays = per_frame * frames;
  // (fewer than four rays per lane at full size: 3072 wavefronts do as well or a little better -- single frames)
  uint64_t cap = rays >= (uint64_t)ctx->traverse_waves * kWave * ctx->small_rays_per_lane ? ctx->traverse_waves
                                                                                           : std::min<uint32_t>(ctx->traverse_waves, ctx->small_waves);
  // (a launch over a run of instances, k_traverse4m: "run_waves" -- room for the other batch's kernels, so only when there is one)
  if (run && ctx->big_slots >= 2) cap = std::min<uint64_t>(cap, ctx->run_waves);
  const uint64_t want = ((rays + kWave - 1u) / kWave + 7u) & ~7ull;
  return (uint32_t)std::min<uint64_t>(cap, std::max<uint64_t>(std::min<uint32_t>(ctx->min_waves, ctx->traverse_waves), want));
}

// launches [k, k + run) of the plan are one traversal launch: consecutive objects that instantiate the same mesh, with
// nothing between them (k_traverse4m; "merge_instances")
size_t launch_run(const ptc_ctx* ctx, size_t k)
{
  size_t run = 1;
  const auto& l = ctx->launches[k];
  if (ctx->trace_variant == 3 && ctx->merge_instances)
    while (k + run < ctx->launches.size() && ctx->launches[k + run].pre_begin == ctx->launches[k + run].pre_end &&
           ctx->launches[k + run].mesh == l.mesh + (uint32_t)run &&
           ctx->object_mesh[ctx->launches[k + run].mesh] == ctx->object_mesh[l.mesh])
      ++run;
  return run;
}

// "roulette" (DESIGN section 5h): does bounce `bounce` of a frame play Russian roulette?  From bounce `roulette` on, never the last
// bounce (capped paths deposit raw throughput as ever); 0 is off.  The kernels that end such a bounce are the roulette instances,
// every other bounce launches what it launched before the parameter existed.
bool roulette_bounce(const ptc_ctx* ctx, int bounce) { return ctx->roulette >= 1 && bounce >= ctx->roulette && bounce < ctx->max_bounces - 1; }
// ... does any bounce of a frame?
bool roulette_frame(const ptc_ctx* ctx) { return ptcd::roulette_frame(ctx->roulette, ctx->max_bounces); }

// The thin lens (ptc_set_lens): is a frame rendered now a lens frame?  Such a frame launches the lens instances of
// ray generation (of the megakernel), and gets no entry points ("beam"): k_beam builds a tile's frustum from the pinhole origin, and
// a lens ray leaves it.  Everything behind the primary ray is per ray and stays as it is.  Radius 0 launches what was launched
// before the lens existed.
bool lens_frame(const ptc_ctx* ctx) { return ctx->lens.radius > 0.0f; }
// ... what the launchers of ray generation get: the context's lens, or the pinhole's "no lens"
DLens frame_lens(const ptc_ctx* ctx) { return lens_frame(ctx) ? ctx->lens : DLens{0.0f, 0.0f}; }

// The environment (ptc_set_environment): a frame rendered now meets the context's map wherever a path leaves the
// scene -- the kernels that end a bounce, a finishing ray generation, the megakernel launch their environment instances (built with
// emitters compiled in: the same bits without any) -- and is not eligible for the persistent launch.  Without a map: what was
// launched before it existed.
bool env_frame(const ptc_ctx* ctx) { return ctx->env.texels != nullptr; }

// ---- the decisions of the launch plan (ptc_ctx::TraceLaunch), each in one place -------------------------------------------

// What opens the object list: a traversal launch with nothing in front of it, a sphere run in front of the first traversal
// launch, or -- a scene without a mesh launch -- nothing (the tail run is all there is).  The first traversal launch walks the
// objects [launches[0].mesh, launches[0].mesh + launch_run(ctx, 0)).
enum class Opens { nothing, launch, spheres };
Opens plan_opens(const ptc_ctx* ctx)
{
  if (ctx->launches.empty()) return Opens::nothing;
  return ctx->launches[0].pre_begin < ctx->launches[0].pre_end ? Opens::spheres : Opens::launch;
}

// "prefold": may a kernel that has a bounce's new rays in registers walk that bounce's leading sphere run for them (k_raygen_next
// for bounce 0, k_shade_fused for the bounce after its own) and leave k_list_flags to open the bounce?  The object list opens
// with a sphere run that would list the rays of the launch behind it -- k_spheres' own conditions: the listing is on, no ray
// sorting -- and the slot has the second set of hit records.  A caller adds what only it knows.
bool may_prefold(const ptc_ctx* ctx, const ptc_ctx::FrameSlot& sl)
{
  return ctx->prefold && ctx->trace_variant == 3 && ctx->fused_shade && ctx->filter_rays && !ctx->ray_sort && sl.next_flags &&
         plan_opens(ctx) == Opens::spheres;
}

// ... and what that kernel gets: the leading sphere run, the objects of the launch behind it, where the hit records and the
// list bytes go
DNextRun next_run(const ptc_ctx* ctx, DHits hits, uint8_t* flags)
{
  const auto& l0 = ctx->launches[0];
  DNextRun next{};
  next.begin = l0.pre_begin;
  next.end = l0.pre_end;
  next.filt_begin = l0.mesh;
  next.filt_end = l0.mesh + (uint32_t)launch_run(ctx, 0);
  next.fold_run = fold_run_of(ctx, l0.pre_begin, l0.pre_end);
  next.hits = hits;
  next.flags = flags;
  return next;
}

// The sphere run that ends the object list, as the kernel that ends a bounce takes it (k_shade_fused, k_persist; k_tail_count
// reads the range alone): the objects [begin, end) -- (0, 0) without such a run, and under the variants 0 / 1, whose trace
// kernel walks the whole list -- and scene.lanes_run / scene.fold_run set for it.
struct ObjectRange {
  uint32_t begin, end;
};
ObjectRange tail_run(const ptc_ctx* ctx, DScene& scene)
{
  const bool tail = ctx->trace_variant == 3 && ctx->tail_begin < ctx->tail_end;
  scene.lanes_run = tail ? lanes_run_of(ctx, ctx->tail_begin, ctx->tail_end) : 0u;
  scene.fold_run = tail && !scene.lanes_run ? fold_run_of(ctx, ctx->tail_begin, ctx->tail_end) : 0u;
  return tail ? ObjectRange{ctx->tail_begin, ctx->tail_end} : ObjectRange{0u, 0u};
}

// Enqueue the traversal launch over launch k of the plan, for the rays in sl.paths[sl.cur]: a run of `run` instances of one mesh
// (k_traverse4m) or one object (k_traverse4; bounce 0's first launch gets the batch's entry points, if batch_begin has made
// any), timed when launches are.  It sets scene.cur and scene.beam.  first: no launch of this bounce has written the hit
// records yet.  pick: the list the lanes fetch their rays through -- sl.worklist (a listed launch), sl.order, or null.
int enqueue_traversal(ptc_ctx* ctx, ptc_ctx::FrameSlot& sl, DScene& scene, size_t k, size_t run, int bounce, bool first, const uint32_t* pick)
{
  const auto& l = ctx->launches[k];
  const bool listed = pick != nullptr && pick == sl.worklist;
  ptc_ctx::TimedLaunch tl;
  if (int rc = timed_begin(ctx, sl.stream, bounce, &tl)) return rc;
  const uint32_t waves = traverse_waves_for(ctx, sl.bi.count, bounce, listed, run > 1);
  scene.cur = ctx->mesh_views[ctx->object_mesh[l.mesh]];  // this object's mesh
  scene.beam = (bounce == 0 && k == 0) ? sl.beam : DBeam{};
  if (run > 1)
    launch_traverse_run(sl.stream, scene, l.mesh, l.mesh + (uint32_t)run, first, sl.paths[sl.cur], sl.hits, bounce, sl.work_slot++ % kWorkSlots,
                        sl.counters, ctx->count_tests, waves, sl.slow_list, pick, sl.bi, listed);
  else
    launch_traverse(sl.stream, scene, l.mesh, first, sl.paths[sl.cur], sl.hits, bounce, sl.work_slot++ % kWorkSlots, sl.counters,
                    ctx->count_tests, waves, sl.slow_list, pick, ctx->trace_variant, sl.bi, listed);
  return timed_end(ctx, sl.stream, tl);
}

// Enqueue raygen for `count` consecutive iterations on the next slot (round robin) and make it the active batch.
int batch_begin(ptc_ctx* ctx, const ptc_ctx::Pending* items, int count)
{
  const int single_slots = (int)ctx->slots.size() - ctx->big_slots;
  const int f = (count == 1 && single_slots > 0) ? ctx->big_slots + (int)(ctx->singles_issued++ % (uint64_t)single_slots)
                                                 : (int)(ctx->batches_issued++ % (uint64_t)ctx->big_slots);
  auto& sl = ctx->slots[(size_t)f];
  // the slot's previous batch has been enqueued on the same stream, so its buffers are free in stream order.
  // A main-stream consumer that still reads the framebuffers (denoise) must finish before anything is folded
  // in: with staging that is only the accumulate at the end of the batch (so tracing overlaps the denoise of
  // the previous frame); without staging the shade kernels write the framebuffers directly.
  if (ctx->main_valid && !ctx->staged) HIP_TRY(ctx, hipStreamWaitEvent(sl.stream, ctx->main_event, 0));
  // launches of different slots run at the same time: each slot has its own stack overflow area
  const size_t spill_need = (size_t)ctx->scene.spill_cap * ctx->scene.spill_stride;
  if (spill_need > sl.spill_elems) {
    HIP_TRY(ctx, hipStreamSynchronize(sl.stream));
    if (sl.spill) HIP_TRY(ctx, hipFree(sl.spill));
    sl.spill = nullptr;
    sl.spill_elems = 0;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&sl.spill), spill_need * sizeof(uint2)));
    sl.spill_elems = spill_need;
  }
  sl.cur = 0;
  sl.work_slot = 0;
  sl.bounces_done = 0;
  sl.prefolded = false;
  sl.bi.count = (uint32_t)count;
  DCameras cams{};
  for (int k = 0; k < count; ++k) {
    cams.c[k] = items[k].cam;
    sl.bi.iteration[k] = items[k].iteration;
  }
  const Opens opens = plan_opens(ctx);
  const uint32_t run0 = opens == Opens::nothing ? 0u : (uint32_t)launch_run(ctx, 0);  // the first traversal launch: this many objects
  // "filter_rays" at bounce 0: when the bounce opens with a traversal launch (no sphere run in front of the first mesh),
  // raygen lists the rays that may hit that launch's world boxes and writes the others' miss records itself
  sl.first_listed = ctx->filter_rays && ctx->trace_variant == 3 && opens == Opens::launch;
  const uint32_t first_mesh = sl.first_listed ? ctx->launches[0].mesh : 0u;
  uint32_t filt_end = sl.first_listed ? first_mesh + run0 : 0u;
  // ... and when that launch is the scene's whole mesh part -- only the sphere run that ends the object list, if any,
  // follows it -- the filter also takes the world boxes of those spheres (the reference tests a sphere's box before the
  // sphere, path_tracer.cu:84): a ray it does not list then hits nothing at all, raygen ends its path, and bounce 0's
  // k_shade_fused walks the list.  (The few rays listed for a sphere's box alone leave the traversal launch at its root.)
  const bool tail = ctx->tail_begin < ctx->tail_end;
  sl.primary_finished = sl.first_listed && ctx->fused_shade && run0 == ctx->launches.size() && (!tail || ctx->tail_begin == filt_end);
  if (sl.primary_finished && tail) filt_end = ctx->tail_end;
  if (may_prefold(ctx, sl)) {
    // "prefold": ray generation walks the leading sphere run for the primary rays itself, and bounce 0 starts with k_list_flags
    // (batch_bounce) instead of k_spheres
    launch_raygen_next(sl.stream, ctx->scene, cams, sl.bi, ctx->band, ctx->pix_count, sl.paths[0], sl.counters,
                       next_run(ctx, sl.hits, sl.next_flags), frame_lens(ctx));
    sl.prefolded = true;
  } else {
    launch_raygen(sl.stream, cams, sl.bi, ctx->band, ctx->pix_count, sl.paths[0], sl.counters, ctx->scene.objects, first_mesh, filt_end,
                  sl.first_listed ? sl.worklist : nullptr, sl.hits, sl.tile_desc, sl.tile_stride, next_epoch(sl), sl.primary_finished,
                  sl.stage, ctx->staged, frame_lens(ctx), ctx->env);
  }
  if (int rc = check_last(ctx, "raygen")) return rc;
  // "beam": when bounce 0 opens with a launch over ONE mesh object (k_traverse4), its primary rays start at entry points
  // computed per tile and distinct camera of the batch (a pinhole batch: lens_frame)
  sl.beam = DBeam{};
  if (ctx->beam && !lens_frame(ctx) && sl.beam_entries && ctx->trace_variant == 3 && opens == Opens::launch && run0 == 1u && ctx->width >= 2u &&
      ctx->height >= 2u) {
    uint8_t cam_of_beam[kMaxBatch];
    uint32_t nbeam = 0;
    for (int k = 0; k < count; ++k) {
      uint32_t b = 0;
      while (b < nbeam && std::memcmp(&cams.c[cam_of_beam[b]], &cams.c[k], sizeof(DCamera)) != 0) ++b;
      if (b == nbeam) cam_of_beam[nbeam++] = (uint8_t)k;
      sl.beam.beam_of[k] = (uint8_t)b;
    }
    DScene scene = ctx->scene;
    const uint32_t mesh_obj = ctx->launches[0].mesh;
    scene.cur = ctx->mesh_views[ctx->object_mesh[mesh_obj]];
    bool cached = sl.beam_count == nbeam && sl.beam_scene == ctx->scene_serial && sl.beam_obj == mesh_obj;
    for (uint32_t b = 0; b < nbeam && cached; ++b) cached = std::memcmp(&sl.beam_cams.c[b], &cams.c[cam_of_beam[b]], sizeof(DCamera)) == 0;
    if (!cached) {
      launch_beam(sl.stream, scene, mesh_obj, cams, cam_of_beam, nbeam, ctx->beam_tiles_x, ctx->beam_tiles_y, ctx->mesh_nodes4[ctx->object_mesh[mesh_obj]],
                  sl.beam_entries);
      if (int rc = check_last(ctx, "beam")) return rc;
      for (uint32_t b = 0; b < nbeam; ++b) sl.beam_cams.c[b] = cams.c[cam_of_beam[b]];
      sl.beam_count = nbeam;
      sl.beam_scene = ctx->scene_serial;
      sl.beam_obj = mesh_obj;
    }
    sl.beam.entries = sl.beam_entries;
    sl.beam.tiles_x = ctx->beam_tiles_x;
    sl.beam.tiles = ctx->beam_tiles_x * ctx->beam_tiles_y;
    sl.beam.width = ctx->width;
    sl.beam.band = ctx->band;
  }
  ctx->active_slot = f;
  return PTC_OK;
}

// One bounce of the active batch: the optional sort, the closest hit launch by launch of the plan, the end of the bounce.
int batch_bounce(ptc_ctx* ctx, int bounce, const uint32_t* slot_base_dev)
{
  auto& sl = ctx->slots[(size_t)ctx->active_slot];
  const bool last = bounce == ctx->max_bounces - 1;
  DPaths in = sl.paths[sl.cur], out = sl.paths[sl.cur ^ 1];
  DScene scene = ctx->scene;
  scene.spill = sl.spill;
  scene.slow_stack = sl.slow_stack;
  const bool persistent = ctx->trace_variant == 3;
  bool wrote = false;  // some launch of this bounce has written the hit records
  const bool prefolded = sl.prefolded;  // ... the previous bounce's shade kernel has, for the leading sphere run ("prefold")
  sl.prefolded = false;

  // ray sorting: the shade kernel of the previous bounce has tagged its surviving rays with their direction octant
  const bool sorted = ctx->ray_sort && persistent && bounce >= 1 && sl.order && !ctx->launches.empty();
  if (sorted) launch_sort_octant(sl.stream, sl.octs, sl.order, ctx->pix_count, bounce, sl.counters, sl.bi);

  if (persistent) {
    // closest hit = the object list walked by the launches of TraceLaunch: per launch of the plan the sphere run in front of it,
    // if there is one (or, behind "prefold", the list that run would have made), then the traversal launch
    for (size_t k = 0; k < ctx->launches.size();) {
      const auto& l = ctx->launches[k];
      const size_t run = launch_run(ctx, k);
      // a sphere run in front of the launch reads every ray anyway: it also lists the rays that may hit one of the launch's
      // objects at all ("filter_rays"), and the launch fetches through that list
      const bool spheres = l.pre_begin < l.pre_end;
      const bool by_spheres = ctx->filter_rays && spheres && !sorted;
      const bool listed = by_spheres || (bounce == 0 && k == 0 && sl.first_listed);  // (bounce 0's first launch: listed by k_raygen)
      if (spheres && k == 0 && prefolded) {
        // "prefold": the shade kernel of the bounce before has walked this run for every survivor and left the hit records
        // (in what is now sl.hits) and one byte per ray; all that is left of k_spheres is its work list
        launch_list_flags(sl.stream, sl.next_flags, ctx->pix_count, bounce, sl.counters, sl.bi, sl.worklist, sl.tile_desc, sl.tile_stride, next_epoch(sl));
        wrote = true;
      } else if (spheres) {
        scene.lanes_run = lanes_run_of(ctx, l.pre_begin, l.pre_end);
        scene.fold_run = fold_run_of(ctx, l.pre_begin, l.pre_end);
        launch_spheres(sl.stream, scene, l.pre_begin, l.pre_end, !wrote, in, sl.hits, ctx->pix_count, bounce, sl.counters, sl.bi,
                       by_spheres ? l.mesh : 0u, by_spheres ? l.mesh + (uint32_t)run : 0u, by_spheres ? sl.worklist : nullptr,
                       sl.tile_desc, sl.tile_stride, by_spheres ? next_epoch(sl) : 0u);
        wrote = true;
      }
      // ("pair_batches": this batch's traversal launches wait for the partner's previous one, and say when they are done)
      if (ctx->turn_mine >= 0 && ctx->turn_wait >= 0) HIP_TRY(ctx, hipStreamWaitEvent(sl.stream, ctx->turn_event[ctx->turn_wait], 0));
      if (int rc = enqueue_traversal(ctx, sl, scene, k, run, bounce, !wrote, listed ? sl.worklist : (sorted ? sl.order : nullptr))) return rc;
      wrote = true;
      if (ctx->turn_mine >= 0) {
        HIP_TRY(ctx, hipEventRecord(ctx->turn_event[ctx->turn_mine], sl.stream));
        ctx->turn_wait = ctx->turn_mine;
      }
      k += run;
    }
  } else {
    // the variants 0 / 1: one kernel walks the whole object list
    ptc_ctx::TimedLaunch tl;
    if (int rc = timed_begin(ctx, sl.stream, bounce, &tl)) return rc;
    launch_trace(sl.stream, scene, in, sl.hits, ctx->pix_count, bounce, sl.counters, ctx->count_tests, ctx->trace_variant);
    wrote = true;
    if (int rc = timed_end(ctx, sl.stream, tl)) return rc;
  }

  // the end of the bounce: the sphere run that ends the object list + the live counts and their scan + the materials
  const ObjectRange tail = tail_run(ctx, scene);
  uint8_t* octs = ctx->ray_sort && !last ? sl.octs : nullptr;
  const bool roulette = roulette_bounce(ctx, bounce);
  if (ctx->fused_shade) {
    // one pass: trailing spheres + material + stable compaction (decoupled look-back) + final gather
    next_epoch(sl);
    // "prefold": the next bounce opens with a sphere run in front of its first traversal launch, which lists its rays -- this
    // kernel walks that run for every survivor (DNextRun)
    const bool prefold = may_prefold(ctx, sl) && !last && wrote;
    const DNextRun next = prefold ? next_run(ctx, sl.hits_other, sl.next_flags) : DNextRun{};
    launch_shade_fused(sl.stream, scene, tail.begin, tail.end, !wrote, in, out, sl.hits, ctx->pix_count, ctx->staged, bounce, last,
                       slot_base_dev, sl.tile_desc, sl.tile_stride, sl.shade_epoch, sl.stage, ctx->band, sl.counters, octs, sl.bi,
                       bounce == 0 && sl.primary_finished ? sl.worklist : nullptr, prefold ? &next : nullptr, ctx->has_emitters, roulette,
                       ctx->env);
    if (prefold) {
      std::swap(sl.hits, sl.hits_other);
      sl.prefolded = true;
    }
  } else {
    launch_tail_count(sl.stream, scene, tail.begin, tail.end, !wrote, in, sl.hits, ctx->pix_count, bounce, sl.chunk_counts, sl.counters,
                      sl.bi, ctx->has_emitters, roulette, slot_base_dev);
    launch_scan(sl.stream, bounce, last, sl.chunk_counts, sl.chunk_offsets, sl.counters, sl.bi);
    launch_shade(sl.stream, scene, in, out, sl.hits, ctx->pix_count, ctx->staged, bounce, last, slot_base_dev,
                 sl.chunk_offsets, sl.stage, ctx->band, sl.counters, octs, sl.bi, ctx->has_emitters, roulette, ctx->env);
  }
  sl.cur ^= 1;
  sl.bounces_done = bounce + 1;
  return check_last(ctx, "bounce");
}

// May the batch that batch_begin has just opened run as bounce 0's traversal launch + ONE persistent launch (k_persist)?
// The launch plan must be the simplest one -- every bounce is one traversal launch over one mesh object with nothing in front
// of it, then the kernel that ends the bounce (a sphere run may end the object list) --, the shade pass the fused one, no ray
// sorting, staged samples, no instrumentation (the counting runs and the per-launch events keep the per-bounce launches:
// same results), no bounce that plays roulette (k_persist is not taught it, section 5h: the per-bounce launches render such a
// frame, with the same bits), no environment (section 5j: the same), and slots must fit the 26 bits a lane keeps them in.
bool persist_ok(const ptc_ctx* ctx, int count)
{
  if (!ctx->persist || ctx->trace_variant != 3 || !ctx->fused_shade || ctx->ray_sort || !ctx->staged || roulette_frame(ctx) || env_frame(ctx)) return false;
  if (ctx->count_tests || ctx->max_bounces < 2 || count < (int)ctx->persist_min_frames) return false;
  if (ctx->launches.size() != 1u || plan_opens(ctx) != Opens::launch || launch_run(ctx, 0) != 1u) return false;
  const auto& sl = ctx->slots[(size_t)ctx->active_slot];
  if (!sl.persist || (uint64_t)sl.bi.stride * (uint64_t)count >= (1ull << kPersistSlotBits)) return false;
  return true;
}

// The batch after raygen: bounce 0's traversal launch as ever (entry points, work list), then the persistent launch for
// everything else -- every shade pass and the traversal of bounces 1 .. max_bounces - 1.
int batch_persist(ptc_ctx* ctx, const uint32_t* slot_base_dev)
{
  auto& sl = ctx->slots[(size_t)ctx->active_slot];
  const int MB = ctx->max_bounces;
  DScene scene = ctx->scene;
  scene.spill = sl.spill;
  scene.slow_stack = sl.slow_stack;
  // bounce 0's closest hit: launch 0 of the plan, one object, the first launch of its bounce, listed if ray generation has listed
  // its rays (persist_ok: the default kernel, no counting run; never one of a pair of batches)
  if (int rc = enqueue_traversal(ctx, sl, scene, /*k*/ 0, /*run*/ 1, /*bounce*/ 0, /*first*/ true, sl.first_listed ? sl.worklist : nullptr)) return rc;
  // everything else (scene.cur stays this object's mesh)
  const auto& l = ctx->launches[0];
  scene.beam = DBeam{};
  const ObjectRange tail = tail_run(ctx, scene);
  DPersistArgs pa{};
  pa.st = sl.persist;
  pa.paths[0] = sl.paths[0];
  pa.paths[1] = sl.paths[1];
  pa.max_bounces = MB;
  pa.service_every = ctx->persist_service_every;
  pa.help_tiles = ctx->persist_help_tiles;
  pa.tail_begin = tail.begin;
  pa.tail_end = tail.end;
  pa.staged = ctx->staged ? 1 : 0;
  pa.slot_base = slot_base_dev;
  pa.tile_desc = sl.tile_desc;
  pa.tile_stride = sl.tile_stride;
  // bounce b's pass: epoch0 + b.  A run that would pass kMaxEpoch starts the new lap early, at 1 (next_epoch clears the descriptors)
  if (sl.shade_epoch + (uint32_t)MB > kMaxEpoch) sl.shade_epoch = kMaxEpoch;
  pa.epoch0 = next_epoch(sl);
  for (int b = 1; b < MB; ++b) next_epoch(sl);
  pa.stage = sl.stage;
  pa.band = ctx->band;
  pa.list0 = sl.primary_finished ? sl.worklist : nullptr;
  pa.slow_list = sl.slow_list;
  ptc_ctx::TimedLaunch tp;  // (reported with bounce 1's launches: bounce 0's traversal launch above has tag 0)
  if (int rc = timed_begin(ctx, sl.stream, 1, &tp)) return rc;
  launch_persist(sl.stream, scene, l.mesh, sl.hits, sl.counters, sl.bi, pa, ctx->traverse_waves, tail.begin < tail.end, pa.list0 != nullptr,
                 ctx->has_emitters);
  if (int rc = timed_end(ctx, sl.stream, tp)) return rc;
  sl.cur = MB & 1;
  sl.bounces_done = MB;
  ++ctx->persist_launches;
  return check_last(ctx, "persistent launch");
}

int batch_end(ptc_ctx* ctx)
{
  auto& sl = ctx->slots[(size_t)ctx->active_slot];
  if (ctx->staged) {
    // fold these samples in after the previous iteration's fold (running means do not commute)
    if (ctx->order_valid) HIP_TRY(ctx, hipStreamWaitEvent(sl.stream, ctx->order_event, 0));
    if (ctx->main_valid) HIP_TRY(ctx, hipStreamWaitEvent(sl.stream, ctx->main_event, 0));
    launch_accumulate(sl.stream, sl.stage, ctx->fb, ctx->pix_count, sl.bi);
    if (int rc = check_last(ctx, "accumulate")) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->order_event, sl.stream));
    ctx->order_valid = true;
  }
  // the live counts of this batch's first frame, for the sizing of later launches (nobody waits for the copy)
  if (sl.live_host && sl.bounces_done == ctx->max_bounces) {
    HIP_TRY(ctx, hipMemcpyAsync(sl.live_host, &sl.counters[0].live[0], sizeof(uint32_t) * 2 * (kMaxBounces + 1), hipMemcpyDeviceToHost, sl.stream));
    sl.live_pending = true;
  }
  HIP_TRY(ctx, hipEventRecord(sl.done, sl.stream));
  ctx->last_slot = ctx->active_slot;
  ctx->active_slot = -1;
  return PTC_OK;
}

// frames per batch ptc_trace may use right now (only the default traversal kernel reads DBatchInfo)
int batch_limit(const ptc_ctx* ctx) { return ctx->staged && ctx->trace_variant == 3 ? ctx->batch : 1; }

// One frame of the megakernel (MegaFrame, pt_device.hpp) from the context, for the slot whose counters it adds to: what the frame's
// options come to in this scene, and for each one what the launch gets -- its data, or the "off" value, written here and nowhere
// else.  launch_megakernel reads the kernel off these values (pt_mega_rules.hpp), so an option that is off must be off here.
// (ctx->env_table: after env_light_table, which an "environment_light" frame with an environment has called.)
MegaFrame mega_frame(const ptc_ctx* ctx, DeviceCounters* counters)
{
  const bool direct = ctx->direct_light && ctx->light_records;  // a lamp table of total weight > 0; without one as with 0
  const bool env = env_frame(ctx);
  const bool env_lit = ctx->environment_light && env && ctx->env_table;  // (section 5k) a map of weight > 0; else as with 0
  const bool smooth = ctx->smooth_normals && ctx->normals_set;           // (section 5n) a scene with vertex normals; else as with 0
  const bool textured = ctx->textures && ctx->textures_set && ctx->texcoords_set;  // (section 5o) textures and coordinates; else as with 0
  // (section 5q) a pool, coordinates and a binding that names a map; else as with 0
  const bool bent = ctx->normal_maps && ctx->textures_set && ctx->texcoords_set && ctx->nmaps_set && ctx->nmap_bound > 0u;
  MegaFrame f{};
  f.scene = ctx->scene;
  f.lights = direct ? DLights{ctx->light_records, ctx->light_thresholds, ctx->light_info.lights, ctx->light_last, ctx->scene.objects,
                              ctx->scene.spheres, ctx->scene.materials}
                    : DLights{};
  f.cam = ctx->cam;
  f.iteration = (uint32_t)ctx->iteration;
  f.band = ctx->band;
  f.pix_count = ctx->pix_count;
  f.max_bounces = ctx->max_bounces;
  f.fb = ctx->fb;
  f.counters = counters;
  f.stats = direct || env_lit || smooth || textured || bent ? ctx->loop_stats : nullptr;  // the frames that count in the loop-counter lines
  f.roulette = mega_rules::roulette_argument(roulette_frame(ctx), ctx->roulette);
  f.lens = frame_lens(ctx);
  f.env = env ? ctx->env : DEnv{nullptr, 0u, 0u};
  f.el = DEnvLight{env_lit ? ctx->env_table : nullptr};
  f.mis = DMis{direct ? ctx->light_material_pdf : nullptr};
  f.sm = DSmooth{smooth ? ctx->vertex_normals : nullptr, ctx->mesh_first_vertex};
  // under a normal map alone the pool and the coordinates without the colour binding: the albedo fetch reads material_texture
  f.tx = textured || bent ? DTex{ctx->tex_texels, ctx->tex_records, textured ? ctx->tex_material : nullptr, ctx->tex_table, ctx->texcoords,
                                 ctx->mesh_first_index}
                          : DTex{};
  f.nm = bent ? DNmap{ctx->nmap_material, ctx->nmap_table} : DNmap{nullptr, nullptr};
  f.emitters = ctx->has_emitters;
  f.weigh = ctx->mis && (direct || env_lit);  // (section 5l) a frame that samples neither light weighs nothing
  return f;
}

}  // namespace

namespace ptcd {
bool roulette_frame(int roulette, int max_bounces) { return roulette >= 1 && roulette < max_bounces - 1; }

// may k_spheres take sphere_fold for the run [begin, end)?  Every object a "simple" sphere (sphere_ball_of)
uint32_t fold_run_of(const ptc_ctx* ctx, uint32_t begin, uint32_t end)
{
  if (!ctx->sphere_fold || end <= begin || end > ctx->sphere_class.size()) return 0u;
  for (uint32_t i = begin; i < end; ++i)
    if (ctx->sphere_class[i] == 0u) return 0u;
  return 1u;
}

// may the sphere run [begin, end) take the per-lane path (sphere_run_lanes)?
uint32_t lanes_run_of(const ptc_ctx* ctx, uint32_t begin, uint32_t end)
{
  if (!ctx->sphere_lanes || end <= begin || end - begin > 8u || end > ctx->sphere_class.size()) return 0u;
  const uint32_t k = ctx->sphere_class[begin];
  if (k == 0u) return 0u;
  for (uint32_t i = begin; i < end; ++i)
    if (ctx->sphere_class[i] != k) return 0u;
  return 1u;
}

// one whole batch on the next slot: raygen, the bounces (per-bounce launches or the persistent launch), the fold
static int enqueue_batch(ptc_ctx* ctx, std::vector<ptc_ctx::Pending>& items)
{
  if (int rc = batch_begin(ctx, items.data(), (int)items.size())) return rc;
  const uint32_t* slot_base = ctx->slot_offset ? ctx->slot_offset_dev : nullptr;
  if (persist_ok(ctx, (int)items.size())) {
    if (int rc = batch_persist(ctx, slot_base)) {
      ctx->active_slot = -1;
      return rc;
    }
    return batch_end(ctx);
  }
  for (int b = 0; b < ctx->max_bounces; ++b)
    if (int rc = batch_bounce(ctx, b, slot_base)) {
      ctx->active_slot = -1;
      return rc;
    }
  return batch_end(ctx);
}

// two batches bounce by bounce on two slots, their traversal launches taking turns ("pair_batches")
static int enqueue_pair(ptc_ctx* ctx, std::vector<ptc_ctx::Pending>& a, std::vector<ptc_ctx::Pending>& b)
{
  for (hipEvent_t& e : ctx->turn_event)
    if (!e) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  const uint32_t* slot_base = ctx->slot_offset ? ctx->slot_offset_dev : nullptr;
  if (int rc = batch_begin(ctx, a.data(), (int)a.size())) return rc;
  const int slot_a = ctx->active_slot;
  if (int rc = batch_begin(ctx, b.data(), (int)b.size())) {
    ctx->active_slot = -1;  // (not the first batch's slot: no failure leaves a batch open)
    return rc;
  }
  const int slot_b = ctx->active_slot;
  ctx->turn_wait = -1;
  int rc = PTC_OK;
  for (int bounce = 0; bounce < ctx->max_bounces && rc == PTC_OK; ++bounce) {
    ctx->active_slot = slot_a;
    ctx->turn_mine = 0;
    rc = batch_bounce(ctx, bounce, slot_base);
    if (rc != PTC_OK) break;
    ctx->active_slot = slot_b;
    ctx->turn_mine = 1;
    rc = batch_bounce(ctx, bounce, slot_base);
  }
  ctx->turn_mine = ctx->turn_wait = -1;
  if (rc != PTC_OK) {
    ctx->active_slot = -1;
    return rc;
  }
  ctx->active_slot = slot_a;
  if (int rc2 = batch_end(ctx)) return rc2;
  ctx->active_slot = slot_b;
  return batch_end(ctx);
}

// enqueue the iterations ptc_trace has queued
int flush_pending(ptc_ctx* ctx, bool from_trace)
{
  if (ctx->pending.empty() && ctx->held.empty()) return PTC_OK;
  if (int rc = bind_device(ctx)) return rc;
  // "pair_batches": a batch that ptc_trace has just filled waits for its partner
  const bool pairing = ctx->pair_batches && ctx->big_slots >= 2 && ctx->staged && ctx->trace_variant == 3 && !ctx->persist;
  if (pairing && from_trace && ctx->held.empty() && (int)ctx->pending.size() >= batch_limit(ctx) && batch_limit(ctx) > 1) {
    ctx->held.swap(ctx->pending);
    return PTC_OK;
  }
  std::vector<ptc_ctx::Pending> first, second;
  first.swap(ctx->held);
  second.swap(ctx->pending);
  if (first.empty()) first.swap(second);
  if (!second.empty() && pairing && first.size() > 1 && second.size() > 1) return enqueue_pair(ctx, first, second);
  if (int rc = enqueue_batch(ctx, first)) return rc;
  if (!second.empty()) return enqueue_batch(ctx, second);
  return PTC_OK;
}

}  // namespace ptcd

extern "C" {
int ptc_trace_begin(ptc_ctx* ctx, const ptc_camera* camera)
{
  if (int rc = frame_ready(ctx)) return rc;
  if (!camera) return fail(ctx, PTC_ERR_INVALID, "camera is NULL");
  if (ctx->active_slot >= 0) return fail(ctx, PTC_ERR_INVALID, "ptc_trace_end missing");
  if (ctx->direct_light) return fail(ctx, PTC_ERR_INVALID, kDirectNeedsMegakernel);  // (the stepwise calls are the streaming loop)
  if (ctx->environment_light) return fail(ctx, PTC_ERR_INVALID, kEnvLightNeedsMegakernel);
  if (ctx->mis) return fail(ctx, PTC_ERR_INVALID, kMisNeedsMegakernel);
  if (ctx->smooth_normals) return fail(ctx, PTC_ERR_INVALID, kSmoothNeedsMegakernel);
  if (ctx->textures) return fail(ctx, PTC_ERR_INVALID, kTexturesNeedMegakernel);
  if (ctx->normal_maps) return fail(ctx, PTC_ERR_INVALID, kNormalMapsNeedMegakernel);
  // (ptc_trace stops at max_iterations; nothing else stands between the stepwise calls and ptc_trace_end's ++iteration)
  if (ctx->iteration == INT_MAX) return fail(ctx, PTC_ERR_INVALID, "the iteration counter is at INT_MAX: ptc_restart or ptc_set_iteration first");
  if (int rc = flush_pending(ctx)) return rc;
  ctx->cam = make_camera(*camera, ctx->width, ctx->height);
  ctx->have_cam = true;
  const ptc_ctx::Pending one{ctx->cam, (uint32_t)ctx->iteration};
  return batch_begin(ctx, &one, 1);
}

int ptc_trace_bounce(ptc_ctx* ctx, int bounce, const uint32_t* slot_base_dev)
{
  if (int rc = frame_ready(ctx)) return rc;
  if (ctx->active_slot < 0) return fail(ctx, PTC_ERR_INVALID, "ptc_trace_begin missing");
  if (bounce < 0 || bounce >= ctx->max_bounces) return fail(ctx, PTC_ERR_INVALID, "bounce out of range");
  if (slot_base_dev) {
    // the slot base was produced by work on the context's stream (the caller's collective): the frame's stream waits
    auto& sl = ctx->slots[(size_t)ctx->active_slot];
    if (sl.stream != ctx->stream) {
      HIP_TRY(ctx, hipEventRecord(ctx->xstream_event, ctx->stream));
      HIP_TRY(ctx, hipStreamWaitEvent(sl.stream, ctx->xstream_event, 0));
    }
  }
  return batch_bounce(ctx, bounce, slot_base_dev);
}

int ptc_trace_end(ptc_ctx* ctx)
{
  if (!ctx || ctx->active_slot < 0) return fail(ctx, PTC_ERR_INVALID, "ptc_trace_begin missing");
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = batch_end(ctx)) return rc;
  ++ctx->iteration;
  ++ctx->frames;
  ctx->result = ctx->fb.color4;  // path_tracer.cu:476
  return PTC_OK;
}

int ptc_live_count_dev(ptc_ctx* ctx, int bounce, const uint32_t** dev_ptr)
{
  if (!ctx || !dev_ptr || bounce < 0 || bounce > (int)kMaxBounces || ctx->slots.empty()) return PTC_ERR_INVALID;
  if (int rc = flush_pending(ctx)) return rc;
  const auto& sl = ctx->slots[(size_t)(ctx->active_slot >= 0 ? ctx->active_slot : ctx->last_slot)];
  *dev_ptr = &sl.counters[sl.bi.count - 1u].live[bounce];  // the most recent iteration of the batch
  return PTC_OK;
}

int ptc_copy_live_count(ptc_ctx* ctx, int bounce, void* dst_dev)
{
  if (!ctx || !dst_dev || bounce < 0 || bounce > (int)kMaxBounces) return PTC_ERR_INVALID;
  if (ctx->active_slot < 0) return fail(ctx, PTC_ERR_INVALID, "ptc_trace_begin missing");
  if (int rc = bind_device(ctx)) return rc;
  auto& sl = ctx->slots[(size_t)ctx->active_slot];
  HIP_TRY(ctx, hipMemcpyAsync(dst_dev, &sl.counters->live[bounce], sizeof(uint32_t), hipMemcpyDeviceToDevice, sl.stream));
  if (sl.stream != ctx->stream) {  // what the caller enqueues on the context's stream next (an all-gather) sees the value
    HIP_TRY(ctx, hipEventRecord(ctx->xstream_event, sl.stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->xstream_event, 0));
  }
  return PTC_OK;
}

int ptc_read_live_count(ptc_ctx* ctx, int bounce, uint32_t* host_out)
{
  if (!ctx || !host_out || bounce < 0 || bounce > (int)kMaxBounces) return PTC_ERR_INVALID;
  if (ctx->active_slot < 0) return fail(ctx, PTC_ERR_INVALID, "ptc_trace_begin missing");
  if (int rc = bind_device(ctx)) return rc;
  auto& sl = ctx->slots[(size_t)ctx->active_slot];
  HIP_TRY(ctx, hipMemcpyAsync(host_out, &sl.counters->live[bounce], sizeof(uint32_t), hipMemcpyDeviceToHost, sl.stream));
  HIP_TRY(ctx, hipStreamSynchronize(sl.stream));
  return PTC_OK;
}

int ptc_trace(ptc_ctx* ctx, const ptc_camera* camera)
{
  if (int rc = frame_ready(ctx)) return rc;
  if (!camera) return fail(ctx, PTC_ERR_INVALID, "camera is NULL");
  if (ctx->active_slot >= 0) return fail(ctx, PTC_ERR_INVALID, "ptc_trace_end missing");
  // "direct_light" is rendered by the megakernel alone: refused before anything is queued or launched
  if (ctx->direct_light && ctx->method != PTC_METHOD_MEGAKERNEL) return fail(ctx, PTC_ERR_INVALID, kDirectNeedsMegakernel);
  if (ctx->direct_light && !ctx->light_error.empty()) return fail(ctx, PTC_ERR_INVALID, ctx->light_error);  // as ptc_direct_light
  if (ctx->environment_light && ctx->method != PTC_METHOD_MEGAKERNEL) return fail(ctx, PTC_ERR_INVALID, kEnvLightNeedsMegakernel);
  if (ctx->mis && ctx->method != PTC_METHOD_MEGAKERNEL) return fail(ctx, PTC_ERR_INVALID, kMisNeedsMegakernel);
  if (ctx->smooth_normals && ctx->method != PTC_METHOD_MEGAKERNEL) return fail(ctx, PTC_ERR_INVALID, kSmoothNeedsMegakernel);
  if (ctx->textures && ctx->method != PTC_METHOD_MEGAKERNEL) return fail(ctx, PTC_ERR_INVALID, kTexturesNeedMegakernel);
  if (ctx->normal_maps && ctx->method != PTC_METHOD_MEGAKERNEL) return fail(ctx, PTC_ERR_INVALID, kNormalMapsNeedMegakernel);
  if (ctx->iteration >= ctx->max_iterations) {  // path_tracer.cu:391
    ctx->result = ctx->fb.color4;
    return PTC_OK;
  }
  if (ctx->method == PTC_METHOD_MEGAKERNEL) {
    // one kernel per sample, accumulating in place: frames are serialised on slot 0's stream
    if (ctx->staged) {
      if (int rc = sync_frames(ctx)) return rc;
    } else if (int rc = flush_pending(ctx)) {
      return rc;
    }
    auto& sl = ctx->slots[0];
    ctx->cam = make_camera(*camera, ctx->width, ctx->height);
    ctx->have_cam = true;
    // "environment_light" (DESIGN section 5k): a frame whose environment has a table, i.e. a map of weight > 0; else as with 0
    if (ctx->environment_light && env_frame(ctx))
      if (int rc = env_light_table(ctx)) return rc;
    const MegaFrame frame = mega_frame(ctx, sl.counters);
    if (frame.stats && ctx->loop_stats_clear) {
      HIP_TRY(ctx, hipMemsetAsync(ctx->loop_stats, 0, kLoopStatBytes, sl.stream));
      ctx->loop_stats_clear = false;
    }
    launch_megakernel(sl.stream, frame);
    if (int rc = check_last(ctx, "megakernel")) return rc;
    HIP_TRY(ctx, hipEventRecord(sl.done, sl.stream));
    if (ctx->staged) {
      HIP_TRY(ctx, hipEventRecord(ctx->order_event, sl.stream));
      ctx->order_valid = true;
    }
    ctx->last_slot = 0;
    sl.bi.count = 1u;
    ++ctx->iteration;
    ++ctx->frames;
    ctx->result = ctx->fb.color4;
    return PTC_OK;
  }
  // streaming mode: queue the iteration; a full batch goes to the GPU
  ctx->cam = make_camera(*camera, ctx->width, ctx->height);
  ctx->have_cam = true;
  ctx->pending.push_back(ptc_ctx::Pending{ctx->cam, (uint32_t)ctx->iteration});
  ++ctx->iteration;
  ++ctx->frames;
  ctx->result = ctx->fb.color4;  // path_tracer.cu:476
  if ((int)ctx->pending.size() >= batch_limit(ctx)) return flush_pending(ctx, true);
  return PTC_OK;
}

}  // extern "C"

