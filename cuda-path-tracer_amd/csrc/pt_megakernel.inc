// pt_megakernel.inc -- k_megakernel, the whole path in one thread.  Included (inside namespace pt, after pt_kernels_common.inc) by
// pt_kernels.hip, which instantiates the plain instances beside the closest-hit kernels as ever, and by pt_mega_direct.hip, which
// instantiates the kRoulette ones: the code object that holds the traversal kernels stays the one it was (DESIGN section 5h).
// path_tracing_mega_kernel, path_tracer.cu:227-269: the whole path in one thread, one RNG stream per
// pixel (a different image from streaming mode at the same seed -- a property of the reference).
// kEmit: the scene has an emissive material (the host's choice; without one the instance is the reference's loop as it was).
// kRoulette: Russian roulette from bounce `roulette` on, the last bounce excepted (DESIGN section 5h; the host picks the instance
// when some bounce plays): after the emitter check and before evaluate_material, on the roulette stream of the pixel.
template <bool kEmit, bool kRoulette = false>
__global__ __launch_bounds__(kWave) void k_megakernel(DScene sc, DCamera cam, uint32_t iteration, DBand band,
                                                      uint32_t pix_count, int max_bounces, DFrame fb,
                                                      DeviceCounters* counters, int roulette)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  const uint32_t s = blockIdx.x * kWave + threadIdx.x;
  uint32_t rays = 0u, flags = 0u;
  if (s < pix_count) {
    const uint32_t pixel = band_pixel(band, s);
    const uint32_t x = pixel % cam.width, y = pixel / cam.width;
    Minstd rng;
    rng.seed(path_seed(pixel, iteration));
    const float fx = (float)x + rng.uniform();
    const float fy = (float)y + rng.uniform();
    Ray ray;
    generate_ray(cam, fx, fy, ray.o, ray.d);
    ray.tmin = 1e-4f;
    ray.tmax = FLT_MAX;
    f3 color = mk3(1.0f, 1.0f, 1.0f);
    f3 normal = -ray.d;
    float depth = 1e6f;
    for (int i = 0; i < max_bounces; ++i) {
      Hit rec;
      rec.t = 0.0f;
      rec.p = rec.n = mk3(0.f, 0.f, 0.f);
      rec.mat = 0u;
      rec.side = 0u;
      ++rays;
      Tally tally;
      if (!ray_scene<false>(ray, sc, rec, s_stack + threadIdx.x, flags, tally)) {
        color = color * background(ray.d);
        break;
      }
      if (i == 0) {
        normal = rec.n;
        depth = rec.t;
      }
      bool tmin_flag = ray.tmin != 1e-4f;
      if (kEmit && is_emitter(sc.materials[rec.mat])) {  // the path ends at the emitter: no draw
        color = emit_color(color, sc.materials[rec.mat]);
        break;
      }
      if (kRoulette && i >= roulette && i != max_bounces - 1 && roulette_ends(color, pixel, iteration, (uint32_t)i)) {
        color = mk3(0.0f, 0.0f, 0.0f);  // the path ends by chance: the sample is 0, no draw
        break;
      }
      evaluate_material(ray.o, ray.d, tmin_flag, rec.p, rec.n, rec.side, sc.materials[rec.mat], rng, color);
      ray.tmin = tmin_flag ? 1e-5f : 1e-4f;
    }
    accumulate_color(fb.color4, s, iteration, color);
    accumulate_nd(fb.nd4, s, iteration, normal, depth);
    if (flags) atomicOr(&counters->flags, flags);
  }
  // one ray-counter atomic per wavefront
  uint32_t sum = rays;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if (threadIdx.x == 0u && sum) atomicAdd(&counters->rays_total, (unsigned long long)sum);
}
