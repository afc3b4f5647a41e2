// pt_mega_direct.hip -- the megakernel's instances off the plain path: k_megakernel_direct (direct lighting),
// k_megakernel<.., true> (Russian roulette, section 5h), k_megakernel_env_light (the environment as a light, section 5k) and the thin lens's k_megakernel_lens / k_megakernel_direct_lens (section 5i),
// with their launchers.  The loop itself, with what kDirect and kRoulette add
// to it, is mega_path (pt_megakernel.inc); the shadow ray's any-hit walk is scene_occluded (pt_kernels_common.inc).  Part of
// libptcore.so.
#include "pt_device.hpp"
#include "pt_rng.hpp"
#include "pt_beam_rules.hpp"
#include "pt_feed_rules.hpp"
#include "pt_light_sample.hpp"
#include "pt_env_light.hpp"
#include <float.h>
#include <limits.h>

namespace pt {

#include "pt_kernels_common.inc"

#include "pt_megakernel.inc"

// path_tracing_mega_kernel (path_tracer.cu:227-269) with DESIGN section 5g's rule: mega_path<true, kRoulette, true>.  One thread per
// pixel of the band; launched only for a scene with a lamp table of total weight > 0 (so the scene has an emissive material).
template <bool kRoulette>
__global__ __launch_bounds__(kWave) void k_megakernel_direct(DScene sc, DLights lt, DCamera cam, uint32_t iteration, DBand band,
                                                             uint32_t pix_count, int max_bounces, DFrame fb,
                                                             DeviceCounters* counters, unsigned long long* stats, int roulette)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  mega_path<true, kRoulette, true>(sc, lt, cam, iteration, band, pix_count, max_bounces, fb, counters, stats, roulette,
                                   s_stack + threadIdx.x);
}

// ... under a thin lens
template <bool kRoulette>
__global__ __launch_bounds__(kWave) void k_megakernel_direct_lens(DScene sc, DLights lt, DCamera cam, uint32_t iteration, DBand band,
                                                                  uint32_t pix_count, int max_bounces, DFrame fb,
                                                                  DeviceCounters* counters, unsigned long long* stats, int roulette, DLens lens)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  mega_path<true, kRoulette, true, true>(sc, lt, cam, iteration, band, pix_count, max_bounces, fb, counters, stats, roulette,
                                         s_stack + threadIdx.x, lens);
}

// ... with an environment: the plain loop and the direct-lit one, each once -- emitters and roulette compiled in
// (mega_path: the same bits without them), pinhole or lens by lens.radius
template <bool kDirect>
__global__ __launch_bounds__(kWave) void k_megakernel_env(DScene sc, DLights lt, DCamera cam, uint32_t iteration, DBand band, uint32_t pix_count,
                                                          int max_bounces, DFrame fb, DeviceCounters* counters, unsigned long long* stats,
                                                          int roulette, DLens lens, DEnv env)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  mega_path<true, true, kDirect, false, true>(sc, lt, cam, iteration, band, pix_count, max_bounces, fb, counters, stats, roulette,
                                              s_stack + threadIdx.x, lens, env);
}

// ... with the environment as a light as well ("environment_light"): one instance -- emitters and roulette compiled
// in, pinhole or lens by lens.radius, the lamps' samples by lt.records
__global__ __launch_bounds__(kWave) void k_megakernel_env_light(DScene sc, DLights lt, DCamera cam, uint32_t iteration, DBand band,
                                                                uint32_t pix_count, int max_bounces, DFrame fb, DeviceCounters* counters,
                                                                unsigned long long* stats, int roulette, DLens lens, DEnv env, DEnvLight el)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  mega_path<true, true, true, false, true, true>(sc, lt, cam, iteration, band, pix_count, max_bounces, fb, counters, stats, roulette,
                                                 s_stack + threadIdx.x, lens, env, el);
}

// the plain megakernel's instances that play roulette (the plain ones: pt_kernels.hip)
void launch_megakernel_roulette(hipStream_t s, const DScene& scene, const DCamera& cam, uint32_t iteration, DBand band, uint32_t pix_count,
                                int max_bounces, DFrame fb, DeviceCounters* counters, bool emitters, int roulette)
{
  const dim3 grid((pix_count + kWave - 1u) / kWave), block(kWave);
  if (emitters)
    hipLaunchKernelGGL((k_megakernel<true, true>), grid, block, 0, s, scene, cam, iteration, band, pix_count, max_bounces, fb, counters, roulette);
  else
    hipLaunchKernelGGL((k_megakernel<false, true>), grid, block, 0, s, scene, cam, iteration, band, pix_count, max_bounces, fb, counters, roulette);
}

// the plain loop under a thin lens: all four instances, the plain ones too -- pt_kernels.hip stays the code object it was
void launch_megakernel_lens(hipStream_t s, const DScene& scene, const DCamera& cam, uint32_t iteration, DBand band, uint32_t pix_count,
                            int max_bounces, DFrame fb, DeviceCounters* counters, bool emitters, int roulette, DLens lens)
{
  const dim3 grid((pix_count + kWave - 1u) / kWave), block(kWave);
  const bool plays = roulette >= 1 && roulette < max_bounces - 1;  // some bounce plays roulette
  if (emitters && plays)
    hipLaunchKernelGGL((k_megakernel_lens<true, true>), grid, block, 0, s, scene, cam, iteration, band, pix_count, max_bounces, fb, counters, roulette, lens);
  else if (emitters)
    hipLaunchKernelGGL((k_megakernel_lens<true, false>), grid, block, 0, s, scene, cam, iteration, band, pix_count, max_bounces, fb, counters, 0, lens);
  else if (plays)
    hipLaunchKernelGGL((k_megakernel_lens<false, true>), grid, block, 0, s, scene, cam, iteration, band, pix_count, max_bounces, fb, counters, roulette, lens);
  else
    hipLaunchKernelGGL((k_megakernel_lens<false, false>), grid, block, 0, s, scene, cam, iteration, band, pix_count, max_bounces, fb, counters, 0, lens);
}

// a frame with an environment (env.texels != null, the caller's check).  lights: the lamp table of a "direct_light" frame, or null
// (DLights::records) for the plain loop; roulette: the context's parameter -- a value that plays at no bounce becomes INT_MAX here
void launch_megakernel_env(hipStream_t s, const DScene& scene, const DLights& lights, const DCamera& cam, uint32_t iteration, DBand band,
                           uint32_t pix_count, int max_bounces, DFrame fb, DeviceCounters* counters, unsigned long long* stats, int roulette,
                           DLens lens, DEnv env)
{
  const dim3 grid((pix_count + kWave - 1u) / kWave), block(kWave);
  const int plays_from = roulette >= 1 && roulette < max_bounces - 1 ? roulette : INT_MAX;
  if (lights.records)
    hipLaunchKernelGGL(k_megakernel_env<true>, grid, block, 0, s, scene, lights, cam, iteration, band, pix_count, max_bounces, fb, counters, stats,
                       plays_from, lens, env);
  else
    hipLaunchKernelGGL(k_megakernel_env<false>, grid, block, 0, s, scene, lights, cam, iteration, band, pix_count, max_bounces, fb, counters, stats,
                       plays_from, lens, env);
}

void launch_megakernel_env_light(hipStream_t s, const DScene& scene, const DLights& lights, const DCamera& cam, uint32_t iteration, DBand band,
                                 uint32_t pix_count, int max_bounces, DFrame fb, DeviceCounters* counters, unsigned long long* stats, int roulette,
                                 DLens lens, DEnv env, DEnvLight el)
{
  const dim3 grid((pix_count + kWave - 1u) / kWave), block(kWave);
  const int plays_from = roulette >= 1 && roulette < max_bounces - 1 ? roulette : INT_MAX;
  hipLaunchKernelGGL(k_megakernel_env_light, grid, block, 0, s, scene, lights, cam, iteration, band, pix_count, max_bounces, fb, counters, stats,
                     plays_from, lens, env, el);
}

void launch_megakernel_direct(hipStream_t s, const DScene& scene, const DLights& lights, const DCamera& cam, uint32_t iteration, DBand band,
                              uint32_t pix_count, int max_bounces, DFrame fb, DeviceCounters* counters, unsigned long long* stats,
                              int roulette, DLens lens)
{
  const dim3 grid((pix_count + kWave - 1u) / kWave), block(kWave);
  if (lens.radius > 0.0f) {  // the thin lens: the same choice, the lens instances
    if (roulette >= 1 && roulette < max_bounces - 1)
      hipLaunchKernelGGL(k_megakernel_direct_lens<true>, grid, block, 0, s, scene, lights, cam, iteration, band, pix_count, max_bounces, fb, counters,
                         stats, roulette, lens);
    else
      hipLaunchKernelGGL(k_megakernel_direct_lens<false>, grid, block, 0, s, scene, lights, cam, iteration, band, pix_count, max_bounces, fb, counters,
                         stats, roulette, lens);
    return;
  }
  if (roulette >= 1 && roulette < max_bounces - 1)  // some bounce plays roulette
    hipLaunchKernelGGL(k_megakernel_direct<true>, grid, block, 0, s, scene, lights, cam, iteration, band, pix_count, max_bounces, fb, counters,
                       stats, roulette);
  else
    hipLaunchKernelGGL(k_megakernel_direct<false>, grid, block, 0, s, scene, lights, cam, iteration, band, pix_count, max_bounces, fb, counters,
                       stats, roulette);
}
}  // namespace pt
