// ptcore_query.cpp -- the ray queries outside the render loop: ptc_intersect_rays (closest hit), ptc_occluded_rays (any hit),
// ptc_direct_light and ptc_environment_light (light sample + shadow ray + resolve: light_query) and the one host path they share: the opening checks, the fast-domain
// rule and the ray packing, the scratch of a traversal launch (WalkScratch), the exact cross-check kernel, and the device memory
// and clean-up of one call (QueryRun).  Part of libptcore.so (ptcore_ctx.hpp).
#include "ptcore_ctx.hpp"

using namespace pt;
using namespace ptcd;

namespace ptcd {

// a query is a batch of one frame of n rays
static DBatchInfo query_batch(uint32_t n)
{
  DBatchInfo bi{};
  bi.stride = n;
  bi.chunk_stride = n / kChunk + 1u;
  bi.count = 1u;
  return bi;
}

// the scratch of a traversal launch over n rays, into the caller's pool (WalkScratch: ptcore_ctx.hpp)
int alloc_walk_scratch(ptc_ctx* ctx, std::vector<void*>& pool, uint32_t n, bool want_chunks, WalkScratch* scr)
{
  int rc = want_chunks ? dev_alloc(ctx, pool, &scr->chunk_counts, query_batch(n).chunk_stride) : PTC_OK;
  if (!rc) rc = dev_alloc(ctx, pool, &scr->slow_list, n);
  if (!rc) rc = dev_alloc(ctx, pool, &scr->slow_stack, (size_t)kStackDepth * kWave);
  if (!rc) rc = dev_alloc(ctx, pool, &scr->spill, (size_t)ctx->scene.spill_cap * ctx->scene.spill_stride);
  if (!rc) rc = dev_alloc(ctx, pool, &scr->counters, 1);
  return rc;
}

// the counters of a query of n rays: zero, and n live rays in its one "frame"
static int begin_walk(ptc_ctx* ctx, hipStream_t stream, const WalkScratch& scr, uint32_t n)
{
  HIP_TRY(ctx, hipMemsetAsync(scr.counters, 0, sizeof(DeviceCounters), stream));
  HIP_TRY(ctx, hipMemcpyAsync(&scr.counters->live[0], &n, sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  return PTC_OK;
}

// the scene as a traversal launch on this scratch takes it
static DScene walk_scene(const ptc_ctx* ctx, const WalkScratch& scr)
{
  DScene scene = ctx->scene;
  scene.spill = scr.spill;
  scene.slow_stack = scr.slow_stack;
  return scene;
}

// persistent wavefronts of a query's traversal launches: about four rays per lane, at most what is resident -- and what the
// overflow area is laid out for
static uint32_t query_waves(const ptc_ctx* ctx, uint32_t n)
{
  return std::min<uint32_t>(ctx->traverse_waves, std::max<uint32_t>(8u, ((n / (4u * kWave)) + 7u) & ~7u));
}

// Occlusion queries on device arrays: rays_o4 = origin.xyz, bits(t_min flag << 31) as in the path state,
// rays_d4 = direction.xyz, t_max; flags = one byte per ray, zeroed here and set to 1 by the kernels.  Every ray must be in the fast
// domain (t_min 1e-4 or 1e-5, t_max >= 0) and the trace variant 3.  Spheres first (one group: any grouping of the object list
// gives the same OR), then one any-hit launch per mesh object; a ray that is already flagged is skipped by every later launch.
// Enqueues only.  The scratch is the caller's: the queries allocate it per call, a bounce loop would lend its slot's.
int occlude_on_device(ptc_ctx* ctx, hipStream_t stream, const float4* rays_o4, const float4* rays_d4, uint32_t n, uint8_t* flags,
                      const WalkScratch& scr, uint32_t* launches)
{
  HIP_TRY(ctx, hipMemsetAsync(flags, 0, n, stream));
  if (int rc = begin_walk(ctx, stream, scr, n)) return rc;
  DScene scene = walk_scene(ctx, scr);
  uint32_t sph_begin = 0xffffffffu, sph_end = 0u;
  auto sphere_run = [&](uint32_t b, uint32_t e) {
    if (b < e) {
      sph_begin = std::min(sph_begin, b);
      sph_end = std::max(sph_end, e);
    }
  };
  for (const auto& l : ctx->launches) sphere_run(l.pre_begin, l.pre_end);
  sphere_run(ctx->tail_begin, ctx->tail_end);
  if (sph_begin < sph_end) {
    launch_occlude_spheres(stream, scene, sph_begin, sph_end, rays_o4, rays_d4, n, flags);
    ++*launches;
  }
  const DBatchInfo bi = query_batch(n);
  const uint32_t waves = query_waves(ctx, n);
  int work_slot = 0;
  for (const auto& l : ctx->launches) {
    scene.cur = ctx->mesh_views[ctx->object_mesh[l.mesh]];
    launch_occlude(stream, scene, l.mesh, rays_o4, rays_d4, flags, work_slot++ % kWorkSlots, scr.counters, waves, scr.slow_list, bi);
    ++*launches;
  }
  return check_last(ctx, "occlusion query");
}

}  // namespace ptcd

namespace {

// The device memory and the two timing events of one query call.  Whatever way the call ends, nothing on ctx->stream may still
// use the pool when it is freed: finish() synchronises after a failure, destroys the events and frees the pool, and the
// destructor does the same for a return that came before it.
struct QueryRun {
  ptc_ctx* ctx;
  const bool timed;  // the caller times its launches, and only while the context's timing is on
  std::vector<void*> pool;
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool finished = false;

  QueryRun(ptc_ctx* c, bool want_timing) : ctx(c), timed(want_timing && c->time_trace) {}
  QueryRun(const QueryRun&) = delete;
  ~QueryRun() { if (!finished) finish(PTC_ERR_HIP); }
  template <typename T>
  int alloc(T** out, size_t count) { return dev_alloc(ctx, pool, out, count); }
  int time_begin()
  {
    if (!timed) return PTC_OK;
    HIP_TRY(ctx, hipEventCreate(&ev[0]));
    HIP_TRY(ctx, hipEventCreate(&ev[1]));
    HIP_TRY(ctx, hipEventRecord(ev[0], ctx->stream));
    return PTC_OK;
  }
  int time_end()
  {
    if (timed) HIP_TRY(ctx, hipEventRecord(ev[1], ctx->stream));
    return PTC_OK;
  }
  // after the stream has been synchronised: adds the time between the two events to *total_ms
  int elapsed_ms(double* total_ms)
  {
    if (!timed) return PTC_OK;
    float ms = 0.0f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ev[0], ev[1]));
    *total_ms += (double)ms;
    return PTC_OK;
  }
  int finish(int rc)
  {
    if (rc != PTC_OK) (void)hipStreamSynchronize(ctx->stream);  // nothing may still use the pool
    for (hipEvent_t& e : ev) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
    free_pool(pool);
    finished = true;
    return rc;
  }
};

constexpr uint32_t kMaxQuery = 0x7fffffffu;  // rays or points of one call

// The checks the three queries open with, in the one order they share: a scene, n == 0 (nothing to do: PTC_OK), the caller's own
// complaint about its arrays (bad_args, if it has one), the size, then the device and the frames ptc_trace has queued -- which
// are enqueued before anything of the query is.  false: the call ends here with *rc.
bool query_prologue(ptc_ctx* ctx, uint32_t n, const char* what, const char* bad_args, int* rc)
{
  *rc = PTC_OK;
  if (!ctx->has_scene) *rc = fail(ctx, PTC_ERR_NO_SCENE, "no scene uploaded");
  else if (n == 0) return false;
  else if (bad_args) *rc = fail(ctx, PTC_ERR_INVALID, bad_args);
  else if (n > kMaxQuery) *rc = fail(ctx, PTC_ERR_INVALID, std::string("too many ") + what);
  else if ((*rc = bind_device(ctx)) == PTC_OK) *rc = flush_pending(ctx);
  return *rc == PTC_OK;
}

// The fast domain: every ray a renderer makes (the path t_min values 1e-4 and 1e-5, a distance >= 0 as t_max) under the default
// trace variant -- what the traversal launches take.  Anything else, and the cross-check variants 0 / 1, takes the exact
// closest-hit kernel (exact_closest_hit).
struct RayClass {
  bool fast, nan_tmax;
};
RayClass classify_rays(const float* rays, uint32_t n, int variant)
{
  RayClass c{variant == 3, false};
  for (uint32_t i = 0; i < n; ++i) {
    const float tmin = rays[8u * (size_t)i + 3u], tmax = rays[8u * (size_t)i + 7u];
    c.fast = c.fast && (tmin == 1e-4f || tmin == 1e-5f) && tmax >= 0.0f;
    c.nan_tmax = c.nan_tmax || tmax != tmax;
  }
  return c;
}

// origin.xyz and the t_min word: in the fast domain the path state's flag bit (set: 1e-5, after a dielectric), else t_min itself
float4 pack_origin(const float* r, bool fast)
{
  float w = r[3];
  if (fast) {
    const uint32_t flag = r[3] == 1e-5f ? 0x80000000u : 0u;
    std::memcpy(&w, &flag, 4);
  }
  return make_float4(r[0], r[1], r[2], w);
}

// direction.xyz and what the kernel the rays go to expects behind it
float4 pack_dir(const float* r, float w) { return make_float4(r[4], r[5], r[6], w); }

// The exact closest-hit kernel, one wavefront per 64 rays, t_min and t_max as floats in o4.w / d4.w: rays outside the fast domain
// and the cross-check variants -- in the reference's order (variant 0) or culled near-first with exact box decisions (variant 1).
void exact_closest_hit(ptc_ctx* ctx, const float4* o4, const float4* d4, uint32_t n, DHits hits, bool reference_order)
{
  launch_intersect(ctx->stream, ctx->scene, o4, d4, n, hits, ctx->misc_counters, reference_order ? 0 : 1);
}

// What ptc_direct_light and ptc_environment_light do behind their own checks and query_prologue: the sample kernel of the caller
// (launch_sample: points, normals, the t_min word, and the three arrays it fills -- shadow rays in the path-state layout, unshadowed
// contributions), the occlusion launches or, under trace variant 0 / 1, the exact closest-hit kernel, then k_light_resolve; the
// caller's counters st.  nothing: there is nothing to sample.  what: the entry point's name, for messages.
template <typename LaunchSample>
int light_query(ptc_ctx* ctx, const float* points, const float* normals, uint32_t n, float* radiance, float* shadow_rays, uint8_t* visible,
                int on_device, bool nothing, ptc_direct_stats& st, const char* what, LaunchSample launch_sample)
{
  int rc;
  const size_t n3 = 3u * (size_t)n;
  if (nothing) {
    // no lamp, or lamps of total weight 0 (no environment table: a map of weight 0): zeros, the empty ray from every point, and no launch
    std::vector<float> rays;
    if (shadow_rays) {
      std::vector<float> pts;
      const float* src = points;
      if (on_device) {
        pts.resize(n3);
        HIP_TRY(ctx, hipMemcpy(pts.data(), points, n3 * sizeof(float), hipMemcpyDeviceToHost));
        src = pts.data();
      }
      rays.assign(8u * (size_t)n, 0.0f);
      for (uint32_t i = 0; i < n; ++i) {
        std::memcpy(&rays[8u * (size_t)i], src + 3u * (size_t)i, 3u * sizeof(float));
        rays[8u * (size_t)i + 3u] = 1e-4f;
      }
    }
    if (on_device) {
      HIP_TRY(ctx, hipMemsetAsync(radiance, 0, n3 * sizeof(float), ctx->stream));
      if (visible) HIP_TRY(ctx, hipMemsetAsync(visible, 0, n, ctx->stream));
      if (shadow_rays) HIP_TRY(ctx, hipMemcpyAsync(shadow_rays, rays.data(), rays.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    } else {
      std::memset(radiance, 0, n3 * sizeof(float));
      if (visible) std::memset(visible, 0, n);
      if (shadow_rays) std::memcpy(shadow_rays, rays.data(), rays.size() * sizeof(float));
    }
    st.points += n;
    return PTC_OK;
  }
  // trace variants 0 / 1 stay cross-checks: the generated rays go through the exact closest-hit kernel, as in ptc_occluded_rays
  // (there t_min travels as a float; a generated t_max is never NaN: d * 0.999f of a finite d, or 0)
  const bool fast = ctx->trace_variant == 3;
  QueryRun q(ctx, true);
  float *d_pts = nullptr, *d_nrm = nullptr, *d_rad = radiance, *d_rays = shadow_rays;
  uint8_t *d_vis = visible, *flags = nullptr;
  float4 *o4 = nullptr, *d4 = nullptr, *contrib = nullptr;
  uint32_t* stats = nullptr;
  DHits hits{};
  WalkScratch scr{};
  rc = q.alloc(&o4, n);
  if (!rc) rc = q.alloc(&d4, n);
  if (!rc) rc = q.alloc(&contrib, n);
  if (!rc) rc = q.alloc(&stats, (size_t)kLightStatLines * 32u);
  if (!rc && !on_device) {
    rc = q.alloc(&d_pts, n3);
    if (!rc) rc = q.alloc(&d_nrm, n3);
    if (!rc) rc = q.alloc(&d_rad, n3);
    if (!rc && shadow_rays) rc = q.alloc(&d_rays, 8u * (size_t)n);
    if (!rc && visible) rc = q.alloc(&d_vis, n);
  }
  if (!rc && fast) {
    rc = q.alloc(&flags, n);
    if (!rc) rc = alloc_walk_scratch(ctx, q.pool, n, false, &scr);
  } else if (!rc) {
    rc = q.alloc(&hits.tp, n);
    if (!rc) rc = q.alloc(&hits.nm, n);
  }
  if (rc) return rc;
  uint32_t launches = 0u, dev_flags = 0u;
  std::vector<uint32_t> host_stats((size_t)kLightStatLines * 32u, 0u);
  auto run = [&]() -> int {
    if (!on_device) {
      HIP_TRY(ctx, hipMemcpyAsync(d_pts, points, n3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(d_nrm, normals, n3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(ctx, hipMemsetAsync(stats, 0, host_stats.size() * sizeof(uint32_t), ctx->stream));
    if (int r2 = q.time_begin()) return r2;
    const float tmin = 1e-4f;
    uint32_t tmin_word = 0u;
    if (!fast) std::memcpy(&tmin_word, &tmin, 4);
    launch_sample(on_device ? points : d_pts, on_device ? normals : d_nrm, tmin_word, o4, d4, contrib);
    ++launches;
    if (fast) {
      if (int r2 = occlude_on_device(ctx, ctx->stream, o4, d4, n, flags, scr, &launches)) return r2;
    } else {
      exact_closest_hit(ctx, o4, d4, n, hits, ctx->trace_variant == 0);
      ++launches;
    }
    launch_light_resolve(ctx->stream, o4, d4, contrib, flags, hits.tp, n, d_rad, d_rays, d_vis, stats);
    ++launches;
    if (int r2 = check_last(ctx, what)) return r2;
    if (int r2 = q.time_end()) return r2;
    if (!on_device) {
      HIP_TRY(ctx, hipMemcpyAsync(radiance, d_rad, n3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
      if (shadow_rays) HIP_TRY(ctx, hipMemcpyAsync(shadow_rays, d_rays, 8u * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
      if (visible) HIP_TRY(ctx, hipMemcpyAsync(visible, d_vis, n, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipMemcpyAsync(host_stats.data(), stats, host_stats.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (fast) HIP_TRY(ctx, hipMemcpyAsync(&dev_flags, &scr.counters->flags, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return q.elapsed_ms(&st.kernel_ms);
  };
  if ((rc = q.finish(run())) != PTC_OK) return rc;
  if (dev_flags & kFlagStackOverflow) return fail(ctx, PTC_ERR_STACK, std::string("traversal stack overflow in ") + what);
  for (uint32_t l = 0; l < kLightStatLines; ++l) {
    st.sampled += host_stats[32u * l];
    st.unoccluded += host_stats[32u * l + 1u];
  }
  st.points += n;
  st.launches += launches;
  return PTC_OK;
}

}  // namespace

extern "C" {

int ptc_intersect_rays(ptc_ctx* ctx, const float* rays, uint32_t n, float* hit_t, float* hit_normal, uint32_t* hit_material,
                       uint8_t* hit_side)
{
  if (!ctx || !rays || !hit_t || !hit_normal || !hit_material || !hit_side) return PTC_ERR_INVALID;
  int rc;
  if (!query_prologue(ctx, n, "rays", nullptr, &rc)) return rc;
  // The default schedule (variant 3) is the production closest-hit stage itself: the object list walked by the
  // traversal launches (k_traverse4 with its sphere runs and its exact redo), fed with the caller's rays instead of
  // path state.
  // Path rays know two t_min values (1e-4, and 1e-5 after a dielectric: a flag bit) and start every bounce with
  // t_max = FLT_MAX; a caller's t_max enters as the "closest hit so far" the segments carry in the hit record.
  // Rays with another t_min take the one-wavefront-per-64-rays kernel with exact box decisions (variant 1).
  const bool path_like = classify_rays(rays, n, ctx->trace_variant).fast;
  constexpr uint32_t kUntouched = 0x7fffffffu;  // material field of a record no segment has written: a miss
  QueryRun q(ctx, false);
  float4 *ro = nullptr, *rd = nullptr;
  DHits hits{};
  WalkScratch scr{};
  rc = q.alloc(&ro, n);
  if (!rc) rc = q.alloc(&rd, n);
  if (!rc) rc = q.alloc(&hits.tp, n);
  if (!rc) rc = q.alloc(&hits.nm, n);
  if (!rc && path_like) rc = alloc_walk_scratch(ctx, q.pool, n, true, &scr);
  if (rc) return rc;
  std::vector<float4> ho(n), hd(n), tp(n), nm(n);
  float untouched_bits;
  std::memcpy(&untouched_bits, &kUntouched, 4);
  for (uint32_t i = 0; i < n; ++i) {
    const float* r = rays + 8u * (size_t)i;
    ho[i] = pack_origin(r, path_like);
    if (path_like) {
      hd[i] = pack_dir(r, 0.0f);
      tp[i] = make_float4(r[7], 0.0f, 0.0f, 0.0f);  // t_max: the closest hit so far
      nm[i] = make_float4(0.0f, 0.0f, 0.0f, untouched_bits);
    } else {
      hd[i] = pack_dir(r, r[7]);
    }
  }
  uint32_t dev_flags = 0u;
  unsigned long long redone = 0ull;
  auto run = [&]() -> int {
    HIP_TRY(ctx, hipMemcpyAsync(ro, ho.data(), n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(rd, hd.data(), n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    if (path_like) {
      HIP_TRY(ctx, hipMemcpyAsync(hits.tp, tp.data(), n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(hits.nm, nm.data(), n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
      if (int r2 = begin_walk(ctx, ctx->stream, scr, n)) return r2;
      DScene scene = walk_scene(ctx, scr);
      const DPaths paths{ro, rd, nullptr};
      const DBatchInfo bi = query_batch(n);
      const uint32_t waves = query_waves(ctx, n);
      int work_slot = 0;
      for (const auto& l : ctx->launches) {
        if (l.pre_begin < l.pre_end) {
          scene.fold_run = fold_run_of(ctx, l.pre_begin, l.pre_end);
          launch_spheres(ctx->stream, scene, l.pre_begin, l.pre_end, false, paths, hits, n, 0, scr.counters, bi);
        }
        scene.cur = ctx->mesh_views[ctx->object_mesh[l.mesh]];
        launch_traverse(ctx->stream, scene, l.mesh, false, paths, hits, 0, work_slot++ % kWorkSlots, scr.counters, false, waves,
                        scr.slow_list, nullptr, ctx->trace_variant, bi);
      }
      launch_tail_count(ctx->stream, scene, ctx->tail_begin, ctx->tail_end, false, paths, hits, n, 0, scr.chunk_counts, scr.counters, bi);
    } else {
      exact_closest_hit(ctx, ro, rd, n, hits, ctx->trace_variant == 0);
    }
    if (int r2 = check_last(ctx, "intersect_rays")) return r2;
    if (path_like) HIP_TRY(ctx, hipMemcpyAsync(&redone, &scr.counters->slow_rays[0], sizeof redone, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(tp.data(), hits.tp, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(nm.data(), hits.nm, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    if (path_like) HIP_TRY(ctx, hipMemcpyAsync(&dev_flags, &scr.counters->flags, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PTC_OK;
  };
  if ((rc = q.finish(run())) != PTC_OK) return rc;
  if (dev_flags & kFlagStackOverflow) return fail(ctx, PTC_ERR_STACK, "traversal stack overflow in ptc_intersect_rays");
  ctx->intersect_redone += redone;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t ms;
    std::memcpy(&ms, &nm[i].w, 4);
    const bool miss = path_like ? (ms & 0x7fffffffu) == kUntouched : tp[i].x < 0.0f;
    hit_t[i] = miss ? -1.0f : tp[i].x;
    hit_normal[3u * i] = nm[i].x;
    hit_normal[3u * i + 1u] = nm[i].y;
    hit_normal[3u * i + 2u] = nm[i].z;
    hit_material[i] = miss ? 0u : (ms & 0x7fffffffu);
    hit_side[i] = miss ? (uint8_t)0 : (uint8_t)(ms >> 31);
  }
  return PTC_OK;
}

// The closest hit's primitive and attributes: k_hit_attributes, one thread per ray on the reference's walk, with
// the scene's vertex normals if any are set.  The rays go up as the caller wrote them, 8 floats each.
int ptc_hit_attributes(ptc_ctx* ctx, const float* rays, uint32_t n, uint32_t* object_out, uint32_t* triangle_out, float* uv_out, float* normal_out)
{
  if (!ctx || !rays || !object_out || !triangle_out || !uv_out || !normal_out) return PTC_ERR_INVALID;
  int rc;
  if (!query_prologue(ctx, n, "rays", nullptr, &rc)) return rc;
  QueryRun q(ctx, false);
  float4* d_rays = nullptr;
  uint32_t *d_obj = nullptr, *d_tri = nullptr, *d_flags = nullptr;
  float2* d_uv = nullptr;
  float* d_nrm = nullptr;
  rc = q.alloc(&d_rays, 2u * (size_t)n);
  if (!rc) rc = q.alloc(&d_obj, n);
  if (!rc) rc = q.alloc(&d_tri, n);
  if (!rc) rc = q.alloc(&d_uv, n);
  if (!rc) rc = q.alloc(&d_nrm, 3u * (size_t)n);
  if (!rc) rc = q.alloc(&d_flags, 1);
  if (rc) return rc;
  uint32_t dev_flags = 0u;
  auto run = [&]() -> int {
    HIP_TRY(ctx, hipMemcpyAsync(d_rays, rays, 8u * (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_flags, 0, sizeof(uint32_t), ctx->stream));
    launch_hit_attributes(ctx->stream, ctx->scene, DSmooth{ctx->normals_set ? ctx->vertex_normals : nullptr, ctx->mesh_first_vertex}, d_rays, n, d_obj,
                          d_tri, d_uv, d_nrm, d_flags);
    if (int r2 = check_last(ctx, "hit_attributes")) return r2;
    HIP_TRY(ctx, hipMemcpyAsync(object_out, d_obj, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(triangle_out, d_tri, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(uv_out, d_uv, n * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(normal_out, d_nrm, 3u * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&dev_flags, d_flags, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PTC_OK;
  };
  if ((rc = q.finish(run())) != PTC_OK) return rc;
  if (dev_flags & kFlagStackOverflow) return fail(ctx, PTC_ERR_STACK, "traversal stack overflow in ptc_hit_attributes");
  return PTC_OK;
}

// what the textured kernels take, from what is set now (a null member: not set)
static DTex textures_of(const ptc_ctx* ctx)
{
  const bool tex = ctx->textures_set;
  return DTex{tex ? ctx->tex_texels : nullptr, tex ? ctx->tex_records : nullptr, tex ? ctx->tex_material : nullptr, ctx->tex_table,
              ctx->texcoords_set ? ctx->texcoords : nullptr, ctx->mesh_first_index};
}

// The interpolated texture coordinate and the albedo at the closest hit: k_hit_surface, ptc_hit_attributes' walk
int ptc_hit_surface(ptc_ctx* ctx, const float* rays, uint32_t n, float* st_out, float* albedo_out)
{
  if (!ctx || !rays || !st_out || !albedo_out) return PTC_ERR_INVALID;
  int rc;
  if (!query_prologue(ctx, n, "rays", nullptr, &rc)) return rc;
  QueryRun q(ctx, false);
  float4* d_rays = nullptr;
  float2* d_st = nullptr;
  float* d_alb = nullptr;
  uint32_t* d_flags = nullptr;
  rc = q.alloc(&d_rays, 2u * (size_t)n);
  if (!rc) rc = q.alloc(&d_st, n);
  if (!rc) rc = q.alloc(&d_alb, 3u * (size_t)n);
  if (!rc) rc = q.alloc(&d_flags, 1);
  if (rc) return rc;
  uint32_t dev_flags = 0u;
  auto run = [&]() -> int {
    HIP_TRY(ctx, hipMemcpyAsync(d_rays, rays, 8u * (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_flags, 0, sizeof(uint32_t), ctx->stream));
    launch_hit_surface(ctx->stream, ctx->scene, textures_of(ctx), d_rays, n, d_st, d_alb, d_flags);
    if (int r2 = check_last(ctx, "hit_surface")) return r2;
    HIP_TRY(ctx, hipMemcpyAsync(st_out, d_st, n * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(albedo_out, d_alb, 3u * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&dev_flags, d_flags, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PTC_OK;
  };
  if ((rc = q.finish(run())) != PTC_OK) return rc;
  if (dev_flags & kFlagStackOverflow) return fail(ctx, PTC_ERR_STACK, "traversal stack overflow in ptc_hit_surface");
  return PTC_OK;
}

// The normal the loop would shade with at the closest hit, from what is set: k_hit_shading_normal, ptc_hit_surface's walk
int ptc_hit_shading_normal(ptc_ctx* ctx, const float* rays, uint32_t n, float* normal_out, uint8_t* outcome_out)
{
  if (!ctx || !rays || !normal_out || !outcome_out) return PTC_ERR_INVALID;
  int rc;
  if (!query_prologue(ctx, n, "rays", nullptr, &rc)) return rc;
  QueryRun q(ctx, false);
  float4* d_rays = nullptr;
  float* d_normal = nullptr;
  uint8_t* d_outcome = nullptr;
  uint32_t* d_flags = nullptr;
  rc = q.alloc(&d_rays, 2u * (size_t)n);
  if (!rc) rc = q.alloc(&d_normal, 3u * (size_t)n);
  if (!rc) rc = q.alloc(&d_outcome, n);
  if (!rc) rc = q.alloc(&d_flags, 1);
  if (rc) return rc;
  uint32_t dev_flags = 0u;
  const DSmooth sm{ctx->normals_set ? ctx->vertex_normals : nullptr, ctx->mesh_first_vertex};
  const DNmap nm{ctx->nmaps_set ? ctx->nmap_material : nullptr, ctx->nmap_table};
  auto run = [&]() -> int {
    HIP_TRY(ctx, hipMemcpyAsync(d_rays, rays, 8u * (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_flags, 0, sizeof(uint32_t), ctx->stream));
    launch_hit_shading_normal(ctx->stream, ctx->scene, sm, textures_of(ctx), nm, d_rays, n, d_normal, d_outcome, d_flags);
    if (int r2 = check_last(ctx, "hit_shading_normal")) return r2;
    HIP_TRY(ctx, hipMemcpyAsync(normal_out, d_normal, 3u * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(outcome_out, d_outcome, n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&dev_flags, d_flags, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PTC_OK;
  };
  if ((rc = q.finish(run())) != PTC_OK) return rc;
  if (dev_flags & kFlagStackOverflow) return fail(ctx, PTC_ERR_STACK, "traversal stack overflow in ptc_hit_shading_normal");
  return PTC_OK;
}

// The lookup of one texture of the pool on the device: k_texture_sample, one thread per coordinate pair
int ptc_sample_texture(ptc_ctx* ctx, uint32_t texture, const float* st, uint32_t n, float* rgb_out, uint8_t* rejected_out)
{
  if (!ctx || !st || !rgb_out) return PTC_ERR_INVALID;
  int rc;
  const bool known = ctx->has_scene && ctx->textures_set && texture < ctx->texture_count;
  const char* bad = known || !ctx->has_scene ? nullptr : (ctx->textures_set ? "ptc_sample_texture: no such texture" : "ptc_sample_texture: no textures are set");
  if (!query_prologue(ctx, n, "coordinates", bad, &rc)) return rc;
  QueryRun q(ctx, false);
  float *d_st = nullptr, *d_rgb = nullptr;
  uint8_t* d_rej = nullptr;
  rc = q.alloc(&d_st, 2u * (size_t)n);
  if (!rc) rc = q.alloc(&d_rgb, 3u * (size_t)n);
  if (!rc) rc = q.alloc(&d_rej, n);
  if (rc) return rc;
  auto run = [&]() -> int {
    HIP_TRY(ctx, hipMemcpyAsync(d_st, st, 2u * (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    launch_texture_sample(ctx->stream, textures_of(ctx), texture, d_st, n, d_rgb, d_rej);
    if (int r2 = check_last(ctx, "texture_sample")) return r2;
    HIP_TRY(ctx, hipMemcpyAsync(rgb_out, d_rgb, 3u * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (rejected_out) HIP_TRY(ctx, hipMemcpyAsync(rejected_out, d_rej, n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PTC_OK;
  };
  return q.finish(run());
}

int ptc_occluded_rays(ptc_ctx* ctx, const float* rays, uint32_t n, uint8_t* occluded)
{
  if (!ctx || !rays || !occluded) return PTC_ERR_INVALID;
  int rc;
  if (!query_prologue(ctx, n, "rays", nullptr, &rc)) return rc;
  // the fast domain: every shadow ray a renderer makes (path t_min values, a distance as t_max).  Anything else -- and the
  // cross-check variants 0 / 1 -- takes the exact closest-hit kernel of ptc_intersect_rays, reduced to a flag on the host.
  // (A NaN t_max: the reference's triangle test rejects on t > t_max, which a NaN never is -- it accepts; the culled walk of
  // variant 1 compares the other way round, so such a call takes the reference-order kernel, variant 0.)
  const RayClass cls = classify_rays(rays, n, ctx->trace_variant);
  const bool fast = cls.fast;
  QueryRun q(ctx, true);
  float4 *ro = nullptr, *rd = nullptr;
  uint8_t* flags = nullptr;
  DHits hits{};
  WalkScratch scr{};
  rc = q.alloc(&ro, n);
  if (!rc) rc = q.alloc(&rd, n);
  if (!rc && fast) {
    rc = q.alloc(&flags, n);
    if (!rc) rc = alloc_walk_scratch(ctx, q.pool, n, false, &scr);
  } else if (!rc) {
    rc = q.alloc(&hits.tp, n);
    if (!rc) rc = q.alloc(&hits.nm, n);
  }
  if (rc) return rc;
  std::vector<float4> ho(n), hd(n);
  for (uint32_t i = 0; i < n; ++i) {
    const float* r = rays + 8u * (size_t)i;
    ho[i] = pack_origin(r, fast);
    hd[i] = pack_dir(r, r[7]);  // t_max travels with the direction, for the any-hit launches and for the exact kernel
  }
  uint32_t launches = 0u, dev_flags = 0u;
  unsigned long long redone = 0ull;
  std::vector<float4> tp;
  auto run = [&]() -> int {
    HIP_TRY(ctx, hipMemcpyAsync(ro, ho.data(), n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(rd, hd.data(), n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    if (int r2 = q.time_begin()) return r2;
    if (fast) {
      if (int r2 = occlude_on_device(ctx, ctx->stream, ro, rd, n, flags, scr, &launches)) return r2;
    } else {
      exact_closest_hit(ctx, ro, rd, n, hits, ctx->trace_variant == 0 || cls.nan_tmax);
      ++launches;
      if (int r2 = check_last(ctx, "occlusion query")) return r2;
    }
    if (int r2 = q.time_end()) return r2;
    if (fast) {
      HIP_TRY(ctx, hipMemcpyAsync(occluded, flags, n, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(&redone, &scr.counters->slow_rays[0], sizeof redone, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(&dev_flags, &scr.counters->flags, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    } else {
      tp.resize(n);
      HIP_TRY(ctx, hipMemcpyAsync(tp.data(), hits.tp, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return q.elapsed_ms(&ctx->occlusion.kernel_ms);
  };
  if ((rc = q.finish(run())) != PTC_OK) return rc;
  if (dev_flags & kFlagStackOverflow) return fail(ctx, PTC_ERR_STACK, "traversal stack overflow in ptc_occluded_rays");
  uint64_t count = 0u;
  if (!fast)
    for (uint32_t i = 0; i < n; ++i) occluded[i] = tp[i].x >= 0.0f ? (uint8_t)1 : (uint8_t)0;
  for (uint32_t i = 0; i < n; ++i) count += occluded[i];
  ctx->occlusion.rays += n;
  ctx->occlusion.occluded += count;
  ctx->occlusion.redone += redone;
  ctx->occlusion.launches += launches;
  return PTC_OK;
}

int ptc_get_occlusion_stats(ptc_ctx* ctx, ptc_occlusion_stats* out)
{
  if (!ctx || !out) return PTC_ERR_INVALID;
  *out = ctx->occlusion;
  return PTC_OK;
}

// Direct-light queries: k_light_sample writes the shadow rays where occlude_on_device takes them -- its first
// caller with rays that were never on the host -- and k_light_resolve combines its flags with the unshadowed contributions.
int ptc_direct_light(ptc_ctx* ctx, const float* points, const float* normals, uint32_t n, uint32_t sample_index, float* radiance,
                     float* shadow_rays, uint8_t* visible, int on_device)
{
  if (!ctx) return PTC_ERR_INVALID;
  // this call's own refusals keep their places among the shared checks: a lamp that cannot be sampled comes after the scene and
  // before n == 0, the NULL arrays after n == 0 (query_prologue's bad_args), the alignment after the size
  if (ctx->has_scene && !ctx->light_error.empty()) return fail(ctx, PTC_ERR_INVALID, ctx->light_error);
  const char* bad_args = nullptr;
  if (!points || !normals || !radiance) bad_args = "points, normals or radiance is NULL";
  else if (n <= kMaxQuery && on_device && shadow_rays && ((uintptr_t)shadow_rays & 15u)) bad_args = "shadow_rays on the device must be 16-byte aligned";
  int rc;
  if (!query_prologue(ctx, n, "points", bad_args, &rc)) return rc;
  const DLights lights{ctx->light_records, ctx->light_thresholds, ctx->light_info.lights, ctx->light_last, ctx->scene.objects, ctx->scene.spheres, ctx->scene.materials};
  return light_query(ctx, points, normals, n, radiance, shadow_rays, visible, on_device, !ctx->light_records, ctx->direct, "ptc_direct_light",
                     [&](const float* pts, const float* nrm, uint32_t tmin_word, float4* o4, float4* d4, float4* contrib) {
                       launch_light_sample(ctx->stream, lights, pts, nrm, n, sample_index, tmin_word, o4, d4, contrib);
                     });
}

int ptc_get_direct_stats(ptc_ctx* ctx, ptc_direct_stats* out)
{
  if (!ctx || !out) return PTC_ERR_INVALID;
  *out = ctx->direct;
  return PTC_OK;
}

// Environment-light queries: ptc_direct_light's path with k_env_light_sample for a sample kernel.  The alias
// table is built here if no call has needed it since the map was set.
int ptc_environment_light(ptc_ctx* ctx, const float* points, const float* normals, uint32_t n, uint32_t sample_index, float* radiance,
                          float* shadow_rays, uint8_t* visible, int on_device)
{
  if (!ctx) return PTC_ERR_INVALID;
  if (!ctx->env.texels) return fail(ctx, PTC_ERR_INVALID, "no environment is set (ptc_set_environment)");
  const char* bad_args = nullptr;
  if (!points || !normals || !radiance) bad_args = "points, normals or radiance is NULL";
  else if (n <= kMaxQuery && on_device && shadow_rays && ((uintptr_t)shadow_rays & 15u)) bad_args = "shadow_rays on the device must be 16-byte aligned";
  int rc;
  if (!query_prologue(ctx, n, "points", bad_args, &rc)) return rc;
  if ((rc = env_light_table(ctx)) != PTC_OK) return rc;
  const DEnv env = ctx->env;
  const DEnvLight el{ctx->env_table};
  return light_query(ctx, points, normals, n, radiance, shadow_rays, visible, on_device, !ctx->env_table, ctx->env_direct, "ptc_environment_light",
                     [&](const float* pts, const float* nrm, uint32_t tmin_word, float4* o4, float4* d4, float4* contrib) {
                       launch_env_light_sample(ctx->stream, env, el, pts, nrm, n, sample_index, tmin_word, o4, d4, contrib);
                     });
}

int ptc_get_environment_light_stats(ptc_ctx* ctx, ptc_environment_light_stats* out)
{
  if (!ctx || !out) return PTC_ERR_INVALID;
  *out = ctx->env_direct;
  return PTC_OK;
}

// The environment's value in the caller's directions: the device function every miss of a frame calls (sky<true>),
// on the context's map.  Queued frames are flushed first; no statistics move.
int ptc_sample_environment(ptc_ctx* ctx, const float* dirs, uint32_t count, float* rgb_out)
{
  if (!ctx) return PTC_ERR_INVALID;
  if (!ctx->env.texels) return fail(ctx, PTC_ERR_INVALID, "no environment is set (ptc_set_environment)");
  if (count == 0u) return PTC_OK;
  if (!dirs || !rgb_out) return fail(ctx, PTC_ERR_INVALID, "dirs or rgb_out is NULL");
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = flush_pending(ctx)) return rc;
  std::vector<void*> pool;
  float *d_dirs = nullptr, *d_out = nullptr;
  int rc = dev_alloc(ctx, pool, &d_dirs, 3u * (size_t)count);
  if (!rc) rc = dev_alloc(ctx, pool, &d_out, 3u * (size_t)count);
  if (rc) {
    free_pool(pool);
    return rc;
  }
  hipError_t e = hipMemcpyAsync(d_dirs, dirs, 3u * (size_t)count * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    launch_env_sample(ctx->stream, ctx->env, d_dirs, count, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(rgb_out, d_out, 3u * (size_t)count * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  free_pool(pool);
  if (e != hipSuccess) return fail(ctx, PTC_ERR_HIP, std::string("sample environment: ") + hipGetErrorString(e));
  return PTC_OK;
}

// The environment sample's solid-angle density in the caller's unit directions: env_light::density, the function a
// miss behind a diffuse vertex calls under "mis", on the context's table -- built here if no call has needed it since the map was set.
// A map of weight 0: zeros, nothing launched.  Queued frames are flushed first; no statistics move.
int ptc_environment_light_pdf(ptc_ctx* ctx, const float* dirs, uint32_t count, float* pdf_out, int on_device)
{
  if (!ctx) return PTC_ERR_INVALID;
  if (!ctx->env.texels) return fail(ctx, PTC_ERR_INVALID, "no environment is set (ptc_set_environment)");
  if (count == 0u) return PTC_OK;
  if (!dirs || !pdf_out) return fail(ctx, PTC_ERR_INVALID, "dirs or pdf_out is NULL");
  if (int rc = bind_device(ctx)) return rc;
  if (int rc = flush_pending(ctx)) return rc;
  if (int rc = env_light_table(ctx)) return rc;
  const DEnvLight el{ctx->env_table};
  const size_t in_bytes = 3u * (size_t)count * sizeof(float), out_bytes = (size_t)count * sizeof(float);
  hipError_t e = hipSuccess;
  if (on_device) {
    if (!el.table) {
      e = hipMemsetAsync(pdf_out, 0, out_bytes, ctx->stream);
    } else {
      launch_env_light_pdf(ctx->stream, el, ctx->env.n, dirs, count, pdf_out);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, PTC_ERR_HIP, std::string("environment light pdf: ") + hipGetErrorString(e));
    return PTC_OK;
  }
  if (!el.table) {
    std::memset(pdf_out, 0, out_bytes);
    return PTC_OK;
  }
  std::vector<void*> pool;
  float *d_dirs = nullptr, *d_out = nullptr;
  int rc = dev_alloc(ctx, pool, &d_dirs, 3u * (size_t)count);
  if (!rc) rc = dev_alloc(ctx, pool, &d_out, (size_t)count);
  if (rc) {
    free_pool(pool);
    return rc;
  }
  e = hipMemcpyAsync(d_dirs, dirs, in_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    launch_env_light_pdf(ctx->stream, el, ctx->env.n, d_dirs, count, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(pdf_out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  free_pool(pool);
  if (e != hipSuccess) return fail(ctx, PTC_ERR_HIP, std::string("environment light pdf: ") + hipGetErrorString(e));
  return PTC_OK;
}

}  // extern "C"
