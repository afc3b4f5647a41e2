// pt_mega_mis.hip -- the megakernel's multiple-importance instance (ptc_set_param "mis"): k_megakernel_mis and
// launch_mega_mis (the rule that names it: pt_mega_rules.hpp), in a translation unit of its own so that pt_mega_direct.hip stays the
// code object it was.  The loop itself, with what kMegaMis adds to it, is mega_path (pt_megakernel.inc); the densities and the weight
// are pt_mis.hpp's and pt_env_light.hpp's.  Part of libptcore.so.
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

// k_megakernel_env_light's shape (pt_mega_direct.hip) with kMis: one instance -- emitters and roulette compiled in, pinhole or lens by
// lens.radius, the lamps' samples by lt.records, the environment's by el.table, the environment itself by env.texels
__global__ __launch_bounds__(kWave) void k_megakernel_mis(DScene sc, DLights lt, DCamera cam, uint32_t iteration, DBand band, uint32_t pix_count,
                                                          int max_bounces, DFrame fb, DeviceCounters* counters, unsigned long long* stats,
                                                          int roulette, DLens lens, DEnv env, DEnvLight el, DMis mis)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  mega_path<kMegaEnvLit | kMegaMis>(sc, lt, cam, iteration, band, pix_count, max_bounces, fb, counters, stats, roulette, s_stack + threadIdx.x, lens,
                                    env, el, mis);
}

void launch_mega_mis(hipStream_t s, const MegaFrame& f, const mega_rules::Instance&)
{
  mega_go_lit(k_megakernel_mis, s, f, f.lens, f.env, f.el, f.mis);
}
}  // namespace pt
