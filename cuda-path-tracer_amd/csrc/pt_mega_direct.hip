// pt_mega_direct.hip -- the megakernel's instances off the plain path: k_megakernel_direct (direct lighting),
// k_megakernel<.., true> (Russian roulette, section 5h), the thin lens's k_megakernel_lens / k_megakernel_direct_lens (section 5i),
// k_megakernel_env (the environment, section 5j) and k_megakernel_env_light (the environment as a light, section 5k), and
// launch_mega_direct, which launches the one of them the instance rule named (pt_mega_rules.hpp).  The loop itself, with what each
// option adds to it, is mega_path (pt_megakernel.inc); the shadow ray's any-hit walk is scene_occluded (pt_kernels_common.inc).
// Part of libptcore.so.
#include "pt_device.hpp"
#include "pt_rng.hpp"
#include "pt_beam_rules.hpp"
#include "pt_feed_rules.hpp"
#include "pt_light_sample.hpp"
#include "pt_env_light.hpp"
#include "pt_mega_rules.hpp"
#include <float.h>
#include <limits.h>

namespace pt {

#include "pt_kernels_common.inc"

#include "pt_megakernel.inc"

// path_tracing_mega_kernel (path_tracer.cu:227-269) with DESIGN section 5g's rule: mega_path with kMegaDirect.  One thread per
// pixel of the band; launched only for a scene with a lamp table of total weight > 0 (so the scene has an emissive material).
template <bool kRoulette>
__global__ __launch_bounds__(kWave) void k_megakernel_direct(DScene sc, DLights lt, DCamera cam, uint32_t iteration, DBand band,
                                                             uint32_t pix_count, int max_bounces, DFrame fb,
                                                             DeviceCounters* counters, unsigned long long* stats, int roulette)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  mega_path<kMegaEmit | kMegaDirect | (kRoulette ? kMegaRoulette : 0u)>(sc, lt, cam, iteration, band, pix_count, max_bounces, fb, counters, stats,
                                                                        roulette, s_stack + threadIdx.x);
}

// ... under a thin lens
template <bool kRoulette>
__global__ __launch_bounds__(kWave) void k_megakernel_direct_lens(DScene sc, DLights lt, DCamera cam, uint32_t iteration, DBand band,
                                                                  uint32_t pix_count, int max_bounces, DFrame fb,
                                                                  DeviceCounters* counters, unsigned long long* stats, int roulette, DLens lens)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  mega_path<kMegaEmit | kMegaDirect | kMegaLens | (kRoulette ? kMegaRoulette : 0u)>(sc, lt, cam, iteration, band, pix_count, max_bounces, fb, counters,
                                                                                    stats, roulette, s_stack + threadIdx.x, lens);
}

// ... with an environment: the plain loop and the direct-lit one, each once -- emitters and roulette compiled in
// (mega_path: the same bits without them), pinhole or lens by lens.radius
template <bool kDirect>
__global__ __launch_bounds__(kWave) void k_megakernel_env(DScene sc, DLights lt, DCamera cam, uint32_t iteration, DBand band, uint32_t pix_count,
                                                          int max_bounces, DFrame fb, DeviceCounters* counters, unsigned long long* stats,
                                                          int roulette, DLens lens, DEnv env)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  mega_path<kMegaEnvBase | (kDirect ? kMegaDirect : 0u)>(sc, lt, cam, iteration, band, pix_count, max_bounces, fb, counters, stats, roulette,
                                                         s_stack + threadIdx.x, lens, env);
}

// ... with the environment as a light as well ("environment_light"): one instance -- emitters and roulette compiled
// in, pinhole or lens by lens.radius, the lamps' samples by lt.records
__global__ __launch_bounds__(kWave) void k_megakernel_env_light(DScene sc, DLights lt, DCamera cam, uint32_t iteration, DBand band,
                                                                uint32_t pix_count, int max_bounces, DFrame fb, DeviceCounters* counters,
                                                                unsigned long long* stats, int roulette, DLens lens, DEnv env, DEnvLight el)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  mega_path<kMegaEnvLit>(sc, lt, cam, iteration, band, pix_count, max_bounces, fb, counters, stats, roulette, s_stack + threadIdx.x, lens, env, el);
}

// this unit's instances, by the rule's result (pt_mega_rules.hpp; in.a, in.b: the kernel's template arguments)
void launch_mega_direct(hipStream_t s, const MegaFrame& f, const mega_rules::Instance& in)
{
  using mega_rules::Kernel;
  switch (in.kernel) {
    case Kernel::plain:  // (the instances that play roulette; the others: pt_kernels.hip)
      return mega_go_plain(in.a ? k_megakernel<true, true> : k_megakernel<false, true>, s, f);
    case Kernel::lens:  // all four instances, the plain ones too
      return mega_go_plain(in.a ? (in.b ? k_megakernel_lens<true, true> : k_megakernel_lens<true, false>)
                                : (in.b ? k_megakernel_lens<false, true> : k_megakernel_lens<false, false>),
                           s, f, f.lens);
    case Kernel::env: return mega_go_lit(in.a ? k_megakernel_env<true> : k_megakernel_env<false>, s, f, f.lens, f.env);
    case Kernel::env_light: return mega_go_lit(k_megakernel_env_light, s, f, f.lens, f.env, f.el);
    case Kernel::direct_lens: return mega_go_lit(in.a ? k_megakernel_direct_lens<true> : k_megakernel_direct_lens<false>, s, f, f.lens);
    case Kernel::direct: return mega_go_lit(in.a ? k_megakernel_direct<true> : k_megakernel_direct<false>, s, f);
    default: return;  // (no kernel of this unit: launch_megakernel does not come here)
  }
}
}  // namespace pt
