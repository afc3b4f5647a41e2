// pt_env.hip -- environment lighting in the streaming loop (ptc_set_environment): the instances of the kernels that
// meet the sky there -- k_raygen_env<true, true> (primary rays that end in ray generation), k_shade_fused_env and k_shade_env (a miss
// at the end of a bounce) -- compiled from the texts the gradient's instances come from (pt_raygen.inc, pt_shade_end.inc), and
// k_env_sample, the lookup on the caller's directions (ptc_sample_environment), and k_env_light_sample, the environment as a light on
// the caller's points (ptc_environment_light, section 5k).  The megakernel's instances: pt_mega_direct.hip.
// The lookup itself: env_rules::lookup (pt_env.hpp) behind sky<true> (pt_kernels_common.inc).  Part of libptcore.so.
//
// The environment instances are built with kEmit on: a scene without an emissive material meets no emitter and gets the same bits, and
// half as many instances are compiled.  kRoulette stays a choice (a kRoulette instance plays at its bounce).
#include "pt_device.hpp"
#include "pt_rng.hpp"
#include "pt_beam_rules.hpp"
#include "pt_feed_rules.hpp"
#include "pt_launch_flags.hpp"
#include "pt_env_light.hpp"
#include <float.h>

namespace pt {

#include "pt_kernels_common.inc"
#include "pt_shade_tile.inc"

#define PT_RAYGEN_LENS 2
#include "pt_raygen.inc"
#undef PT_RAYGEN_LENS

#define PT_SHADE_ENV 1
#include "pt_shade_end.inc"
#undef PT_SHADE_ENV

// ptc_sample_environment: sky<true> on `count` directions of three floats, three floats out each
__global__ __launch_bounds__(256) void k_env_sample(DEnv env, const float* dirs, uint32_t count, float* out)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= count) return;
  const f3 v = sky<true>(mk3(dirs[3u * (size_t)i], dirs[3u * (size_t)i + 1u], dirs[3u * (size_t)i + 2u]), env);
  out[3u * (size_t)i] = v.x;
  out[3u * (size_t)i + 1u] = v.y;
  out[3u * (size_t)i + 2u] = v.z;
}

void launch_env_sample(hipStream_t s, DEnv env, const float* dirs, uint32_t count, float* out)
{
  hipLaunchKernelGGL(k_env_sample, dim3(div_up(count, 256u)), dim3(256), 0, s, env, dirs, count, out);
}

// ptc_environment_light's sample kernel: one thread per point, env_light::sample_point on the point's own stream;
// out in k_light_sample's layout, for the occlusion launches and k_light_resolve (pt_light.hip).  No LDS, no cross-lane work.
__global__ __launch_bounds__(256) void k_env_light_sample(DEnv env, DEnvLight el, const float* __restrict__ points, const float* __restrict__ normals,
                                                          uint32_t n, uint32_t sample_index, uint32_t tmin_word, float4* __restrict__ o4,
                                                          float4* __restrict__ d4, float4* __restrict__ contrib)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const f3 p = mk3(points[3u * (size_t)i], points[3u * (size_t)i + 1u], points[3u * (size_t)i + 2u]);
  const f3 nrm = mk3(normals[3u * (size_t)i], normals[3u * (size_t)i + 1u], normals[3u * (size_t)i + 2u]);
  const env_light::Sample s = env_light::sample_point(el.table, env.texels, env.n, nrm, i, sample_index, 0u);
  o4[i] = make_float4(p.x, p.y, p.z, __uint_as_float(tmin_word));
  d4[i] = make_float4(s.w.x, s.w.y, s.w.z, s.tmax);
  contrib[i] = make_float4(s.contrib.x, s.contrib.y, s.contrib.z, s.sampled ? 1.0f : 0.0f);
}

void launch_env_light_sample(hipStream_t s, DEnv env, DEnvLight el, const float* points, const float* normals, uint32_t n, uint32_t sample_index,
                             uint32_t tmin_word, float4* o4, float4* d4, float4* contrib)
{
  hipLaunchKernelGGL(k_env_light_sample, dim3(div_up(n, 256u)), dim3(256), 0, s, env, el, points, normals, n, sample_index, tmin_word, o4, d4,
                     contrib);
}

// ptc_environment_light_pdf's kernel: one thread per unit direction, env_light::density -- one 16-byte load of the
// table entry the direction falls in (square_of clamps the square into the table).  No LDS, no cross-lane work.
__global__ __launch_bounds__(256) void k_env_light_pdf(DEnvLight el, uint32_t n, const float* __restrict__ dirs, uint32_t count,
                                                       float* __restrict__ pdf)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= count) return;
  pdf[i] = env_light::density(el.table, n, mk3(dirs[3u * (size_t)i], dirs[3u * (size_t)i + 1u], dirs[3u * (size_t)i + 2u]));
}

void launch_env_light_pdf(hipStream_t s, DEnvLight el, uint32_t n, const float* dirs, uint32_t count, float* pdf)
{
  hipLaunchKernelGGL(k_env_light_pdf, dim3(div_up(count, 256u)), dim3(256), 0, s, el, n, dirs, count, pdf);
}

// launch_raygen's finishing form (a listed first launch that walks the whole object list) under an environment
void launch_raygen_env(hipStream_t s, const DCameras& cams, const DBatchInfo& bi, DBand band, uint32_t pix_count, DPaths paths,
                       DeviceCounters* counters, const DObject* objects, uint32_t filt_begin, uint32_t filt_end, uint32_t* worklist, DHits hits,
                       unsigned long long* tile_desc, uint32_t tile_stride, uint32_t epoch, DFrame fb, bool staged, DLens lens, DEnv env)
{
  const dim3 grid(div_up(pix_count, 256u * kListPer) * bi.count), block(256);
  const DTileScan scan{tile_desc, epoch};
  hipLaunchKernelGGL((k_raygen_env<true, true>), grid, block, 0, s, cams, bi, band, pix_count, paths, counters, objects, filt_begin, filt_end,
                     worklist, hits, scan, tile_stride, fb, staged ? 1 : 0, lens, env);
}

void launch_shade_env(hipStream_t s, const DScene& scene, DPaths in, DPaths out, DHits hits, uint32_t max_paths, bool staged, int bounce,
                      bool last_bounce, const uint32_t* slot_base, const uint32_t* chunk_offsets, DFrame fb, DBand band, DeviceCounters* counters,
                      uint8_t* octs, const DBatchInfo& bi, bool roulette, DEnv env)
{
  with_flags(
      [&](auto kRoulette) {
        hipLaunchKernelGGL((k_shade_env<true, decltype(kRoulette)::value>), dim3(div_up(max_paths, 256u), bi.count), dim3(256), 0, s, scene, in, out,
                           hits, staged ? 1 : 0, bounce, last_bounce ? 1 : 0, slot_base, chunk_offsets, fb, band, counters, octs, bi, env);
      },
      roulette);
}

// launch_shade_fused's choices (pt_shade.hip), the environment's instances
void launch_shade_fused_env(hipStream_t s, const DScene& scene, uint32_t obj_begin, uint32_t obj_end, bool first, DPaths in, DPaths out, DHits hits,
                            uint32_t max_paths, bool staged, int bounce, bool last_bounce, const uint32_t* slot_base, unsigned long long* tile_desc,
                            uint32_t tile_stride, uint32_t epoch, DFrame fb, DBand band, DeviceCounters* counters, uint8_t* octs,
                            const DBatchInfo& bi, const uint32_t* list, const DNextRun* next, bool roulette, DEnv env)
{
  const dim3 grid(div_up(max_paths, kFuseTile) * bi.count), block(256);
  const DNextRun none{};
  const bool prefold = next && !first && !last_bounce;
  with_flags(
      [&](auto kSpheres, auto kFirst, auto kNext, auto kRoulette) {
        if constexpr (!(decltype(kFirst)::value && decltype(kNext)::value))
          hipLaunchKernelGGL((k_shade_fused_env<decltype(kSpheres)::value, decltype(kFirst)::value, decltype(kNext)::value, true, decltype(kRoulette)::value>),
                             grid, block, 0, s, scene, obj_begin, obj_end, in, out, hits, staged ? 1 : 0, bounce, last_bounce ? 1 : 0, slot_base,
                             tile_desc, tile_stride, epoch, fb, band, counters, octs, bi, list, next ? *next : none, env);
      },
      obj_begin < obj_end, first && !prefold, prefold, roulette);
}
}  // namespace pt
