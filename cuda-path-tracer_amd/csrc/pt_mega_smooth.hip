// pt_mega_smooth.hip -- smooth shading (ptc_set_vertex_normals, ptc_set_param "smooth_normals"): the megakernel's
// two smooth instances, k_megakernel_smooth<kMis>, and the primitive query's kernel, k_hit_attributes, with launch_mega_smooth (the
// rule that names an instance: pt_mega_rules.hpp) and the query's launcher -- in a translation unit of its own so that every other
// code object stays what it was.  The loop itself, with what kMegaSmooth adds to it, is mega_path (pt_megakernel.inc); the rule is
// pt_smooth.hpp's; the closest hit that reports its winner is ray_scene<.., true> (pt_kernels_common.inc).  Part of libptcore.so.
#include "pt_device.hpp"
#include "pt_rng.hpp"
#include "pt_beam_rules.hpp"
#include "pt_feed_rules.hpp"
#include "pt_light_sample.hpp"
#include "pt_env_light.hpp"
#include "pt_smooth.hpp"
#include "pt_mega_rules.hpp"
#include <float.h>
#include <limits.h>

namespace pt {

#include "pt_kernels_common.inc"

#include "pt_megakernel.inc"

// k_megakernel_mis's shape with kSmooth, with the balance heuristic and without: emitters and roulette compiled in, pinhole or lens by
// lens.radius, the lamps' samples by lt.records, the environment's by el.table, the environment itself by env.texels -- two
// instances render everything the megakernel renders without vertex normals
template <bool kMis>
__global__ __launch_bounds__(kWave) void k_megakernel_smooth(DScene sc, DLights lt, DCamera cam, uint32_t iteration, DBand band, uint32_t pix_count,
                                                             int max_bounces, DFrame fb, DeviceCounters* counters, unsigned long long* stats,
                                                             int roulette, DLens lens, DEnv env, DEnvLight el, DMis mis, DSmooth sm)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  mega_path<kMegaEnvLit | kMegaSmooth | (kMis ? kMegaMis : 0u)>(sc, lt, cam, iteration, band, pix_count, max_bounces, fb, counters, stats, roulette,
                                                                s_stack + threadIdx.x, lens, env, el, mis, sm);
}

// ptc_hit_attributes: one thread per ray, the reference's walk in the reference's order on the thread's column of the LDS stack (no
// claim about speed: the production walk reports no primitive).  A miss: object and triangle 0xffffffff, zeros.
__global__ __launch_bounds__(kWave) void k_hit_attributes(DScene sc, DSmooth sm, const float4* rays, uint32_t n, uint32_t* object_out,
                                                          uint32_t* triangle_out, float2* uv_out, float* normal_out, uint32_t* flags_out)
{
  __shared__ uint32_t s_stack[kStackDepth * kWave];
  const uint32_t r = blockIdx.x * kWave + threadIdx.x;
  if (r >= n) return;
  const float4 ro = rays[2u * (size_t)r], rd = rays[2u * (size_t)r + 1u];
  Ray ray;
  ray.o = xyz(ro);
  ray.tmin = ro.w;
  ray.d = xyz(rd);
  ray.tmax = rd.w;
  Hit rec;
  rec.t = 0.0f;
  rec.p = rec.n = mk3(0.f, 0.f, 0.f);
  rec.mat = 0u;
  rec.side = 0u;
  HitAttr at;
  Tally tally;
  uint32_t flags = 0u;
  uint32_t object = kNoChild, triangle = kNoChild;
  float2 uv = make_float2(0.0f, 0.0f);
  f3 hn = mk3(0.0f, 0.0f, 0.0f);
  if (ray_scene<false, true>(ray, sc, rec, s_stack + threadIdx.x, flags, tally, &at)) {
    object = at.object;
    hn = rec.n;
    if (at.first != kNoChild) {
      triangle = at.first / 3u;
      uv = make_float2(at.u, at.v);
      if (sm.normals) {
        const uint32_t mesh = sc.object_mesh[at.object];
        const uint32_t* idx = sc.mesh_views[mesh].indices + at.first;
        const float* vn = sm.normals + 3u * (size_t)sm.mesh_first_vertex[mesh];
        const f3 n0 = ld3(vn + 3u * (size_t)idx[0]), n1 = ld3(vn + 3u * (size_t)idx[1]), n2 = ld3(vn + 3u * (size_t)idx[2]);
        (void)smooth::shading_normal(n0, n1, n2, at.u, at.v, rec.n, ray.d, sc.objects[at.object].inv_m, hn);
      }
    }
  }
  object_out[r] = object;
  triangle_out[r] = triangle;
  uv_out[r] = uv;
  normal_out[3u * (size_t)r] = hn.x;
  normal_out[3u * (size_t)r + 1u] = hn.y;
  normal_out[3u * (size_t)r + 2u] = hn.z;
  if (flags) atomicOr(flags_out, flags);
}

void launch_mega_smooth(hipStream_t s, const MegaFrame& f, const mega_rules::Instance& in)
{
  mega_go_lit(in.a ? k_megakernel_smooth<true> : k_megakernel_smooth<false>, s, f, f.lens, f.env, f.el, f.mis, f.sm);
}

void launch_hit_attributes(hipStream_t s, const DScene& scene, DSmooth sm, const float4* rays, uint32_t n, uint32_t* object_out,
                           uint32_t* triangle_out, float2* uv_out, float* normal_out, uint32_t* flags)
{
  const dim3 grid((n + kWave - 1u) / kWave), block(kWave);
  hipLaunchKernelGGL(k_hit_attributes, grid, block, 0, s, scene, sm, rays, n, object_out, triangle_out, uv_out, normal_out, flags);
}
}  // namespace pt
