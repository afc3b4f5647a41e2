// pt_raygen.inc -- the ray-generation kernels, k_raygen<kFilter, kFinish> and k_raygen_next.  Included TWICE by pt_shade.hip (inside
// namespace pt, after pt_kernels_common.inc and pt_shade_tile.inc): with PT_RAYGEN_LENS 0 it defines the pinhole kernels under those
// names, with PT_RAYGEN_LENS 1 the thin lens's (DESIGN section 5i) as k_raygen_lens<kFilter, kFinish> and k_raygen_next_lens, which
// take a trailing DLens and call primary_ray<true>; everything behind the primary ray is the same text.  (An include and not a
// device function both kernels call: inlined one level down the pinhole kernels came out with other instructions -- the xors of
// path_seed associated differently -- and the pinhole instances are to stay the ones they were.)
// A third time by pt_env.hip, with PT_RAYGEN_LENS 2: the environment's k_raygen_env<kFilter, kFinish> (ptc_set_environment, DESIGN
// section 5j), whose finishing miss takes sky<true>(d, env).  It takes a trailing DLens and DEnv and serves pinhole and lens alike
// (lens.radius > 0 decides per launch: primary_ray<true> or primary_ray, each its own operations); only <true, true> touches the
// sky, so only that instance exists, and k_raygen_next, which touches none, has no environment form.
#if PT_RAYGEN_LENS == 2
#define PT_RAYGEN_NAME(name) name##_env
#define PT_RAYGEN_LENS_PARAM , DLens lens, DEnv env
#define PT_RAYGEN_PRIMARY(cam, pixel, iteration, rng, ray)                          \
  do {                                                                              \
    if (lens.radius > 0.0f) primary_ray<true>(cam, pixel, iteration, rng, ray, lens); \
    else primary_ray(cam, pixel, iteration, rng, ray);                              \
  } while (0)
#define PT_RAYGEN_SKY(d) sky<true>(d, env)
#elif PT_RAYGEN_LENS
#define PT_RAYGEN_NAME(name) name##_lens
#define PT_RAYGEN_LENS_PARAM , DLens lens
#define PT_RAYGEN_PRIMARY(cam, pixel, iteration, rng, ray) primary_ray<true>(cam, pixel, iteration, rng, ray, lens)
#define PT_RAYGEN_SKY(d) background(d)
#else
#define PT_RAYGEN_NAME(name) name
#define PT_RAYGEN_LENS_PARAM
#define PT_RAYGEN_PRIMARY(cam, pixel, iteration, rng, ray) primary_ray(cam, pixel, iteration, rng, ray)
#define PT_RAYGEN_SKY(d) background(d)
#endif

// raygen_kernel, ray_gen.cu:11-32.  Slot s of this context holds pixel band_pixel(band, s).
// kFilter ("filter_rays"): the bounce's first launch is a traversal launch over the mesh objects [filt_begin, filt_end)
// (no sphere run in front of it): the rays that may hit one of their world boxes go on its work list, the others get
// their miss record here (what that launch would have written for them) -- the sky pixels of an outdoor scene never
// reach the traversal kernel.
// kFinish (with kFilter, when that launch walks the scene's WHOLE object list): a ray that is not listed hits nothing at
// all, so its path ends here -- throughput (1, 1, 1) times the sky into the frame, exactly what the shade kernel does
// for a miss at bounce 0 (path_tracer.cu:304-307, ray_gen.cu:26-28) -- and neither its ray nor a miss record is written;
// bounce 0's k_shade_fused then walks the work list instead of all slots.  Per sky pixel and frame: 32 bytes written
// here instead of 48, and 48 bytes the shade kernel no longer reads.
template <bool kFilter, bool kFinish>
__global__ __launch_bounds__(256) void PT_RAYGEN_NAME(k_raygen)(DCameras cams, DBatchInfo bi, DBand band, uint32_t pix_count,
                                                DPaths paths, DeviceCounters* counters, const DObject* objects, uint32_t filt_begin,
                                                uint32_t filt_end, uint32_t* worklist, DHits hits, DTileScan scan, uint32_t tile_stride,
                                                DFrame fb, int staged PT_RAYGEN_LENS_PARAM)
{
  const uint32_t frame = blockIdx.x % bi.count;  // see DBatchInfo; frame-fastest: neighbouring workgroups take their tickets on different lines
  const DCamera& cam = cams.c[frame];
  const uint32_t iteration = bi.iteration[frame];
  paths.o4 += (size_t)frame * bi.stride;  // (written out, not offset_frame: with it k_raygen<true, true> orders its scalar adds differently)
  paths.d4 += (size_t)frame * bi.stride;
  counters += frame;
  scan.desc += (size_t)frame * tile_stride;
  if (kFinish && staged) {
    fb.color4 += (size_t)frame * bi.stride;
    fb.nd4 += (size_t)frame * bi.stride;
  }
  const uint32_t acc_iteration = staged ? 0u : iteration;
  const uint32_t tiles = gridDim.x / bi.count;
  const uint32_t tile = kFilter ? list_tile(counters, tiles) : blockIdx.x / bi.count;
  const uint32_t block_first = tile * (256u * kListPer);  // a workgroup generates kListPer x 256 consecutive slots
  if (tile == 0u) {
    if (threadIdx.x == 0u) counters->live[0] = pix_count;
    // fetch cursors of this frame's persistent traversal launches
    for (uint32_t i = threadIdx.x; i < (uint32_t)kWorkSlots * 8u; i += 256u) (&counters->work[0][0][0])[i * 32u] = 0u;
  }
  uint32_t may_mask = 0u;
#pragma unroll
  for (int j = 0; j < kListPer; ++j) {
    const uint32_t s = block_first + (uint32_t)j * 256u + threadIdx.x;
    if (s >= pix_count) continue;
    const uint32_t pixel = band_pixel(band, s);
    Minstd rng;
    Ray ray;
    PT_RAYGEN_PRIMARY(cam, pixel, iteration, rng, ray);
    const f3 o = ray.o, d = ray.d;
    bool may_hit = true;
    if (kFilter) {
      may_hit = may_hit_boxes(objects, filt_begin, filt_end, o, d, FLT_MAX);
      may_mask |= may_hit ? 1u << j : 0u;
    }
    if (kFinish && !may_hit) {
      const uint32_t local_pixel = band_local(band, pixel);
      const f3 color = mk3(1.0f, 1.0f, 1.0f) * PT_RAYGEN_SKY(d);
      accumulate_nd(fb.nd4, local_pixel, acc_iteration, -d, 1e6f);
      accumulate_color(fb.color4, local_pixel, acc_iteration, color);
      continue;
    }
    stnt(&paths.o4[s], make_float4(o.x, o.y, o.z, __uint_as_float(pixel)));
    stnt(&paths.d4[s], make_float4(d.x, d.y, d.z, 0.0f));
    // (the throughput of a primary ray is (1, 1, 1), ray_gen.cu:25: the shade kernels know that at bounce 0 and neither
    // is it written here nor read there -- 32 bytes per pixel and frame less)
    if (kFilter && !may_hit) stnt(&hits.tp[(size_t)frame * bi.stride + s], make_float4(-1.0f, 0.f, 0.f, 0.f));
  }
  if (kFilter) list_rays(may_mask, worklist, counters, (size_t)frame * bi.stride, tile, tiles, scan);
}

// "prefold" at bounce 0: ray generation for a scene whose object list opens with a sphere run in front of a mesh (config 2).  The
// primary ray is in registers: k_spheres<first, filter>'s work for it -- the run, the hit or miss record, the byte that says
// whether it goes on the mesh launch's work list (shade_tile<.., kNext> does the same for the later bounces) -- is done here, and
// bounce 0 starts with k_list_flags.
#if PT_RAYGEN_LENS != 2
__global__ __launch_bounds__(256) void PT_RAYGEN_NAME(k_raygen_next)(DScene sc, DCameras cams, DBatchInfo bi, DBand band, uint32_t pix_count, DPaths paths,
                                                     DeviceCounters* counters, DNextRun next PT_RAYGEN_LENS_PARAM)
{
  const uint32_t frame = blockIdx.x % bi.count;
  const DCamera& cam = cams.c[frame];
  const uint32_t iteration = bi.iteration[frame];
  const size_t fo = (size_t)frame * bi.stride;
  offset_frame(paths, fo);
  offset_frame(next.hits, fo);
  next.flags += fo;
  counters += frame;
  const uint32_t tile = blockIdx.x / bi.count;
  const uint32_t block_first = tile * (256u * kListPer);
  if (tile == 0u) {
    if (threadIdx.x == 0u) counters->live[0] = pix_count;
    for (uint32_t i = threadIdx.x; i < (uint32_t)kWorkSlots * 8u; i += 256u) (&counters->work[0][0][0])[i * 32u] = 0u;
  }
#pragma unroll 1
  for (int j = 0; j < kListPer; ++j) {
    const uint32_t s = block_first + (uint32_t)j * 256u + threadIdx.x;
    if (s >= pix_count) continue;
    const uint32_t pixel = band_pixel(band, s);
    Minstd rng;
    Ray ray;
    PT_RAYGEN_PRIMARY(cam, pixel, iteration, rng, ray);  // (t_min as load_ray reads it: the sign bit of a primary ray's pixel word is clear)
    stnt(&paths.o4[s], make_float4(ray.o.x, ray.o.y, ray.o.z, __uint_as_float(pixel)));
    stnt(&paths.d4[s], make_float4(ray.d.x, ray.d.y, ray.d.z, 0.0f));
    Hit rec;
    bool changed = false;
    if (next.fold_run != 0u) sphere_fold(sc, next.begin, next.end, ray, rec, changed);
    else sphere_segment<true>(sc, next.begin, next.end, ray, rec, changed);
    if (changed) store_hit(next.hits, s, rec);
    else stnt(&next.hits.tp[s], make_float4(-1.0f, 0.f, 0.f, 0.f));
    next.flags[s] = may_hit_boxes(sc.objects, next.filt_begin, next.filt_end, ray.o, ray.d, ray.tmax) ? (uint8_t)1 : (uint8_t)0;
  }
}
#endif

#undef PT_RAYGEN_NAME
#undef PT_RAYGEN_SKY
#undef PT_RAYGEN_LENS_PARAM
#undef PT_RAYGEN_PRIMARY
